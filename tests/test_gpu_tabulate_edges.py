"""GPU: csrc/gk_tabulate.hip at the limits of its own data structures, against the restatement on records of
tests/tabulate_reference.py (itself pinned to oracle/tabulate.py and to the reference-made fixtures by
tests/test_tabulate_reference_host.py).  Every sample is tabulated three ways -- from the 128-byte records, from the compact
words, and from the records under GK_TEST_HOOKS=two_walks -- and every exposed field (counts, offsets, ids, pair sources,
genes, NH, novel keys) must equal the restatement's, bit for bit.  Every case first proves from the restatement's per-mate
diagnostics that it sits on the edge it names.

The edges, read from the launch arithmetic of the file:

* events: pass 1 (tab_count) keeps a mate's event words 0 .. 3 in registers (kEvRegs = 4, one uint4 per mate) and 4 .. 21 in
  the overflow row ev_more (GK_MAX_EVENTS = 22); window_negatives clears the positives of the register words in one
  unrolled loop and those of ev_more in another.  A 23rd event is refused (wk.overflow, GK_ERR_CAPACITY).
* staged head: the first kHeadWords = 16 words of a record are staged in LDS, i.e. the header, the 7 CIGAR words and
  mismatch words 0 .. 5; mismatches 6 .. 15 and the inserted-string ids come from global memory.
* window: the kept bits of candidates 0 .. 127 ride in registers (kMaskRegs = 4), 128 .. 255 in the overflow row
  (kMaskWords = 8); one window beyond 256 candidates sends the whole sample to the second walk (tab_emit).  Deletions are
  found through del_bits, read as two words joined at lo % 32; the table has two words of padding.  A mate with an N takes
  the candidate-by-candidate loop.
* bounds: lb_a / lb_t hold last variant position + 2 entries per gene and clamp beyond; snp_ord is read only below the
  last entry; insertions and deletions go through the 16-base bucket table, whose last bucket closes the gene.
* tab_expand: a wave takes 64 mates = 32 pairs, a workgroup two waves; a wave whose run of lists is at most kExpandCap =
  4096 ids assembles it in LDS, a longer one writes directly; a wide pair's slots are left to tab_emit_wide.
* cooperative_negatives (tab_emit): the windows of a wave's 64 mates laid end to end and walked 64 candidates a step.
* novel ranks: first appearance (mate << 16 | event) through one word of event bits per mate, kWideWords words per wide
  mate; a hash table of 2^novel_log2cap slots with linear probing that wraps.
* correction table: applied where gene_pos0[ref] + pos < gene_pos0[ref + 1]."""
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tabulate_reference import CapacityError, hash64, makeKey, tabulateRecords  # noqa: E402

from kir_graph_amd._lib import CIG_D, CIG_I, CIG_M, CIG_S, MATE_DTYPE, MATE_WIDE_DTYPE, SPILLED, GkError  # noqa: E402
from kir_graph_amd.index import GkIndex  # noqa: E402
from kir_graph_amd.msa2hisat import Variant  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("counts", "off", "ids", "pair_src", "pair_gene", "pair_nh", "novel_key")
ROUTES = ("records", "compact", "two_walks")
KA, KB, KC = "KIRA*BACKBONE", "KIRB*BACKBONE", "KIRC*BACKBONE"      # genes 0, 1, 2
INS_STRINGS = ["AA", "AC", "AG", "AT", "CA", "CC"]                   # string ids 0 .. 5 of the index
_OPS = {"M": CIG_M, "I": CIG_I, "D": CIG_D, "S": CIG_S}
A, C_, G, T, N = (ord(c) for c in "ACGTN")


def exposed(tab) -> dict:
    """Everything a tabulation exposes (as in test_gpu_tabulate_compact.py)."""
    return {"counts": np.array([tab.n_pairs, tab.n_valid, tab.n_ids, tab.n_novel, int(tab.info.err_flags)]),
            "off": tab.offsets().copy(), "ids": tab.ids().copy(), "pair_src": tab.pairSrc().copy(),
            "pair_gene": tab.pairGene().copy(), "pair_nh": tab.pairNH().copy(), "novel_key": tab.novelKeys().copy()}


# ------------------------------------------------------------------------------------------------ the index
def _v(ref, pos, typ, val):
    return Variant(pos=pos, typ=typ, ref=ref, val=val, allele=[ref.split("*")[0] + "*001"])


@lru_cache(maxsize=None)
def dense_index() -> GkIndex:
    """Three genes, 3500 variants or so.

    KIRA: the substitution to C at every position of [0, 1500) and [1600, 3500) -- below 1500 a variant's ordinal is its
    position, [1500, 1600) is a hole without variants --, the substitution to G as well on [2000, 2100), the insertions
    INS_STRINGS[k] at 2600 + 10 k, a deletion of 4 at 2800, deletions of 1, 2 and 3 at 3000.
    KIRB: no variant.
    KIRC: the substitution to C at 0, 5, .., 200 (its last variant position); insertion AA + deletion of 2 at 15, at 100 and at
    192; insertion AC + deletion of 3 at 16; at 120 an insertion AA, the substitutions to A, C and G and a deletion of 2."""
    vs = [_v(KA, p, "single", "C") for p in list(range(1500)) + list(range(1600, 3500))]
    vs += [_v(KA, p, "single", "G") for p in range(2000, 2100)]
    vs += [_v(KA, 2600 + 10 * k, "insertion", s) for k, s in enumerate(INS_STRINGS)]
    vs += [_v(KA, 2800, "deletion", 4)] + [_v(KA, 3000, "deletion", n) for n in (1, 2, 3)]
    vs += [_v(KC, p, "single", "C") for p in range(0, 201, 5)]
    for p in (15, 100, 192):
        vs += [_v(KC, p, "insertion", "AA"), _v(KC, p, "deletion", 2)]
    vs += [_v(KC, 16, "insertion", "AC"), _v(KC, 16, "deletion", 3)]
    vs += [_v(KC, 120, "insertion", "AA"), _v(KC, 120, "single", "A"), _v(KC, 120, "single", "G"), _v(KC, 120, "deletion", 2)]
    vs.sort()
    for i, v in enumerate(vs):
        v.id = f"hv{i}"
    gidx = GkIndex.fromVariants(vs, genes=[KA, KB, KC])
    assert gidx.genes == [KA, KB, KC] and gidx.ins_strings == INS_STRINGS
    assert gidx.gene_vbeg[1] == gidx.gene_vbeg[2] and gidx.n_variant < 5000        # KIRB has none
    return gidx


@lru_cache(maxsize=None)
def tail_index(n_var: int) -> GkIndex:
    """One gene: the substitution to C at 0 .. n_var - 2 and, as the LAST variant, a deletion of 1 at n_var - 2."""
    vs = [_v(KA, p, "single", "C") for p in range(n_var - 1)] + [_v(KA, n_var - 2, "deletion", 1)]
    vs.sort()
    gidx = GkIndex.fromVariants(vs, genes=[KA])
    assert gidx.n_variant == n_var and (int(gidx.key[-1]) >> 30) & 3 == 2
    return gidx


def ordinal(gidx, ref, pos, typ, val) -> int:
    """The ordinal of an index variant (it must exist)."""
    k = makeKey(ref, pos, typ, val)
    i = int(np.searchsorted(gidx.key, np.uint64(k)))
    assert i < gidx.n_variant and int(gidx.key[i]) == k, (ref, pos, typ, val)
    return i


# ------------------------------------------------------------------------------------------------ records
def mate(pos0, cigar, mms=(), ins=(), ref=0, flag=3, nm=0, nh=1):
    """One gk_mate: ``mms`` = [(reference offset from pos0, base)], ``ins`` = string ids of the I operations."""
    r = np.zeros(1, dtype=MATE_DTYPE)
    ops = [(int(n) << 4) | _OPS[o] for n, o in re.findall(r"(\d+)([MIDS])", cigar)]
    r["pos0"], r["flag"], r["ref"], r["nh"], r["nm"] = pos0, flag, ref, nh, nm
    r["n_cig"], r["n_mm"], r["n_ins"] = len(ops), len(mms), len(ins)
    r["cig"][0, :len(ops)] = ops
    for i, (o, b) in enumerate(mms):
        r["mm"]["ref_off"][0, i], r["mm"]["base"][0, i] = o, ord(b)
    r["ins"][0, :len(ins)] = list(ins)
    return r


def wide_mate(pos0, cigar, mms=(), ins=(), ref=0, flag=3, nm=0, nh=1):
    r = np.zeros(1, dtype=MATE_WIDE_DTYPE)
    ops = [(int(n) << 4) | _OPS[o] for n, o in re.findall(r"(\d+)([MIDS])", cigar)]
    r["pos0"], r["flag"], r["ref"], r["nh"], r["nm"] = pos0, flag, ref, nh, nm
    r["n_cig"], r["n_mm"], r["n_ins"] = len(ops), len(mms), len(ins)
    r["cig"][0, :len(ops)] = ops
    r["mm"][0, :len(mms)] = [(o << 8) | ord(b) for o, b in mms]
    r["ins"][0, :len(ins)] = list(ins)
    return r


def hole(k=0):
    """A mate in KIRA's hole: no event, an empty window."""
    return mate(1510 + k % 40, "30M")


def ordinary(k):
    """100 bases of KIRA below 1500 with a known substitution and a novel one; the words differ from mate to mate."""
    return mate(40 + 13 * (k % 97), "100M", [(7 + k % 11, "C"), (40 + k % 23, "G")], nh=1 + k % 3)


def known_only(k):
    return mate(40 + 13 * (k % 97), "100M", [(7 + k % 11, "C"), (40 + k % 23, "C")])


def sample(pairs):
    return np.ascontiguousarray(np.concatenate([m for pair in pairs for m in pair]))


def around(items, n_pairs=40, filler=ordinary):
    """``items`` (mates) among ordinary pairs: item j is mate 2 * (3 + 4 j) + (j & 1), its partner a mate of the hole.
    Returns (records, [mate index of every item])."""
    pairs = [(filler(2 * i), filler(2 * i + 1)) for i in range(max(n_pairs, 4 * len(items) + 4))]
    at = []
    for j, m in enumerate(items):
        p = 3 + 4 * j
        pairs[p] = (m, hole(j)) if j % 2 == 0 else (hole(j), m)
        at.append(2 * p + (j & 1))
    return sample(pairs), at


def spill_of(rec, wide_pairs):
    """``wide_pairs`` {pair: (left wide mate, right wide mate)}: the heads in ``rec`` and the arrays Tabulation takes."""
    wide, which = [], []
    for k, p in enumerate(sorted(wide_pairs)):
        for side in (0, 1):
            w = wide_pairs[p][side]
            head = np.zeros(1, dtype=MATE_DTYPE)
            for f in ("pos0", "flag", "ref", "nh", "nm"):
                head[f] = w[f]
            head["n_cig"] = SPILLED
            head["ins"][0, 0] = k
            rec[2 * p + side] = head[0]
            wide.append(w)
        which.append(p)
    return np.concatenate(wide), np.array(which, dtype=np.int64)


def tabulate3(device, monkeypatch, gidx, rec, spill=None, correction=None, hooks="", routes=ROUTES):
    """The restatement's result and {route: the pass-2 kernel that ran}; asserts that every route equals the restatement."""
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.packed import CompactMates
    assert len(rec) <= 2 * 700 and gidx.n_variant < 5000
    want = tabulateRecords(rec, gidx, spill=spill, correction=correction)
    dindex = DeviceIndex(device, gidx)
    ran = {}
    device.profEnable(True)
    try:
        for how in routes:
            monkeypatch.setenv("GK_TEST_HOOKS", ",".join(h for h in (hooks, "two_walks" if how == "two_walks" else "") if h))
            device.profCollect()
            tab = Tabulation(dindex, CompactMates(rec, threads=2) if how == "compact" else rec, dev=device, spill=spill,
                             correction=correction)
            prof = device.profCollect()
            ran[how] = sorted(k for k in ("tab_emit", "tab_expand") if k in prof)
            got = exposed(tab)
            tab.mates.free()
            tab.close()
            for f in FIELDS:
                same = np.array_equal(got[f], want[f])
                where = None
                if not same and len(got[f]) == len(want[f]):
                    where = int(np.flatnonzero(np.asarray(got[f]) != np.asarray(want[f]))[0])
                assert same, (how, f, len(got[f]), len(want[f]), where)
    finally:
        monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
        device.profEnable(False)
        dindex.close()
    if "two_walks" in ran and len(rec):
        assert ran["two_walks"] == ["tab_emit"]
    return want, ran


def in_window(d, e):
    return e["known"] and d["lo"] <= e["ordinal"] < d["hi"]


# ------------------------------------------------------------------------------------------------ event storage
def _six_ins(mms, ins=(0, 1, 2, 3, 4, 5), n=6):
    """KIRA 2590: 10 bases, then ``n`` insertions of 2 at 2600, 2610, .., 10 bases after each, 20 after the last."""
    cigar = "10M" + "2I10M" * (n - 1) + "2I20M"
    return mate(2590, cigar, mms, list(ins)[:n])


def _mm(n, novel=(), base_n=(), step=5, first=1):
    """``n`` mismatches at offsets first, first + step, ..: C (known) unless listed as novel (G) or N."""
    return [(first + step * i, "N" if i in base_n else "G" if i in novel else "C") for i in range(n)]


EVENT_CASES = {
    "0 events": lambda: mate(200, "120M"),
    "1 event": lambda: mate(200, "120M", _mm(1)),
    "4 events": lambda: mate(200, "120M", _mm(4)),
    "5 events, 3 and 4 known": lambda: mate(200, "120M", _mm(5)),
    "5 events, 4 novel": lambda: mate(200, "120M", _mm(5, novel=(4,))),
    "21 events": lambda: _six_ins(_mm(15)),
    "22 events, 21 novel": lambda: _six_ins(_mm(16, novel=(15,))),
    "22 events, all known": lambda: _six_ins(_mm(16)),
    "N as event 0": lambda: mate(1990, "120M", [(15, "N"), (40, "C")]),
    "N as event 5": lambda: mate(1990, "120M", _mm(5) + [(40, "N")]),
}


@pytest.mark.parametrize("case", list(EVENT_CASES))
def test_event_words_in_registers_and_in_the_overflow_row(device, monkeypatch, case):
    gidx = dense_index()
    rec, (at,) = around([EVENT_CASES[case]()])
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at]
    ev = d["events"]
    assert d["walked"] and not d["dropped"] and not d["clipped"] and d["n_pos"] == d["n_events"]
    if case[0].isdigit():
        assert d["n_events"] == int(case.split()[0])
    if case == "5 events, 3 and 4 known":      # the last register word and the first word of ev_more, both candidates
        assert in_window(d, ev[3]) and in_window(d, ev[4]) and d["n_neg"] == d["hi"] - d["lo"] - 5
    elif case == "5 events, 4 novel":
        assert in_window(d, ev[3]) and not ev[4]["known"] and d["n_neg"] == d["hi"] - d["lo"] - 4
    elif case == "21 events":
        assert all(in_window(d, e) for e in ev) and sum(e["typ"] == 0 for e in ev) == 6
    elif case == "22 events, 21 novel":
        assert not ev[21]["known"] and ev[21]["typ"] == 1 and all(e["known"] for e in ev[:21])
    elif case == "22 events, all known":      # 16 mismatches and 6 insertions
        assert sum(e["typ"] == 1 for e in ev) == 16 and sum(e["typ"] == 0 for e in ev) == 6 and all(in_window(d, e) for e in ev)
        assert d["n_neg"] == d["hi"] - d["lo"] - 22
    elif case.startswith("N as event"):
        k = int(case.split()[-1])
        assert ev[k]["is_n"] and not ev[k]["known"] and d["any_n"] and d["n_events"] == k + (2 if k == 0 else 1)
        both = [ordinal(gidx, 0, ev[k]["pos"], 1, b) for b in (C_, G)]      # the position carries two index substitutions
        ids = want["ids"].tolist()
        assert d["lo"] <= both[0] < both[1] < d["hi"] and d["n_neg"] == d["hi"] - d["lo"] - 2 - (d["n_events"] - 1)
        assert not set(both) & set(ids[want["off"][0]:])      # ... which no list of the sample names (no other mate is there)


def test_a_23rd_event_is_refused(device, monkeypatch):
    """16 mismatches and 7 adjacent I / D operations in 8 CIGAR operations: the restatement raises, the library returns
    GK_ERR_CAPACITY from its checked path (wk.overflow) on every route."""
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.packed import CompactMates
    gidx = dense_index()
    big = mate(200, "80M1I1D1I1D1I1D1I", _mm(16), ins=[0, 1, 2, 3])
    rec, _ = around([big])
    with pytest.raises(CapacityError):
        tabulateRecords(rec, gidx)
    dindex = DeviceIndex(device, gidx)
    for how in ROUTES:
        monkeypatch.setenv("GK_TEST_HOOKS", "two_walks" if how == "two_walks" else "")
        with pytest.raises(GkError, match="more variant events"):
            Tabulation(dindex, CompactMates(rec, threads=2) if how == "compact" else rec, dev=device)
    monkeypatch.delenv("GK_TEST_HOOKS")
    ok, _ = around([mate(200, "80M1I1D1I1D1I1D", _mm(16), ins=[0, 1, 2])])      # 22: taken
    want, _ = tabulate3(device, monkeypatch, gidx, ok)
    assert max(d.get("n_events", 0) for d in want["mates"]) == 22
    dindex.close()


# ------------------------------------------------------------------------------------------------ staged head
def _head_mates():
    bases = "GACCGCCAGCAGCGAC"      # mismatches 5 and 6 are C: known
    def mm(n, step, first):
        return [(first + step * i, bases[i]) for i in range(n)]
    return [mate(300, "120M", mm(6, 7, 3)), mate(310, "120M", mm(7, 7, 4)), mate(305, "120M", mm(16, 7, 5)),
            mate(330, "120M", mm(7, 7, 6)), mate(290, "120M", mm(16, 7, 2)), mate(340, "120M", mm(6, 7, 1))]


def test_mismatches_on_both_sides_of_the_staged_head(device, monkeypatch):
    """Mates of 6, 7 and 16 mismatches in adjacent lanes, mismatches 5 and 6 known, every neighbour with other words at
    the same offsets."""
    gidx = dense_index()
    ms = _head_mates()
    pairs = [(ordinary(i), ordinary(i + 1)) for i in range(20)]
    pairs[5:8] = [(ms[0], ms[1]), (ms[2], ms[3]), (ms[4], ms[5])]
    rec = sample(pairs)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    ds = want["mates"][10:16]
    assert [d["n_events"] for d in ds] == [6, 7, 16, 7, 16, 6]
    for d in ds:
        assert d["events"][5]["known"] and in_window(d, d["events"][5]) and d["n_pos"] == d["n_events"]
        assert d["n_events"] < 7 or in_window(d, d["events"][6])
        assert any(not e["known"] for e in d["events"])
    words = rec[10:16].view(np.uint32).reshape(6, 32)
    for w in range(10, 26):      # a mismatch word differs from the same word of either neighbour lane
        col = words[:, w].tolist()
        assert all(a != b for a, b in zip(col, col[1:]) if a or b), w


@pytest.mark.parametrize("ids,dropped", [((0, 1, 2, 3, 4, 5), False), ((0, 9, 2, 7, 4, 5), True), ((5, 4, 3, 2, 1, 0), True)])
def test_six_inserted_strings_from_global_memory(device, monkeypatch, ids, dropped):
    gidx = dense_index()
    rec, at = around([_six_ins(_mm(3), ins=ids), _six_ins(_mm(2), ins=(0, 1, 2, 3, 4, 5)), _six_ins([], ins=ids, n=3)])
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at[0]]
    assert d["n_events"] == 9 and d["dropped"] == dropped and sum(e["typ"] == 0 for e in d["events"]) == 6
    assert [e["known"] for e in d["events"] if e["typ"] == 0] == [i == k for k, i in enumerate(ids)]
    assert not want["mates"][at[1]]["dropped"] and want["mates"][at[1]]["n_pos"] == 8


# ------------------------------------------------------------------------------------------------ window and kept bits
SIZES = [0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257]
WINDOWS = [(0, None), (1, None)] + [(n, r) for n in SIZES[2:] for r in (0, 1, 31)]


@pytest.mark.parametrize("n,r", WINDOWS)
def test_window_lengths_and_their_first_bit(device, monkeypatch, n, r):
    """A window of exactly n candidates that starts at ordinal = r (mod 32), with a known event in its first word and one in
    its last.  257 sends the sample to tab_emit on every route; 256 does not."""
    gidx = dense_index()
    if n == 0:
        target = mate(1520, "40M")
    elif n == 1:
        target = mate(1590, "10M")                      # right edge 1600: the substitution at 1600 alone
    else:
        s = n - 1
        target = mate(320 + r, f"{s}M", [(1, "C")] + ([(s - 2, "C")] if s >= 4 else []))
    rec, (at,) = around([target], filler=known_only)
    want, ran = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at]
    assert d["hi"] - d["lo"] == n and (r is None or d["lo"] % 32 == r)
    assert d["n_neg"] == n - d["n_events"] and all(in_window(d, e) for e in d["events"])
    widest = max(m["hi"] - m["lo"] for m in want["mates"] if m["walked"])
    assert widest == max(n, 101)
    assert ran["records"] == ran["compact"] == (["tab_emit"] if n > 256 else ["tab_expand"])


@pytest.mark.parametrize("n_var", [64, 65, 95])
def test_window_that_ends_at_the_last_ordinal(device, monkeypatch, n_var):
    """n_var % 32 = 0, 1, 31: the last word of del_bits and its padding; the last variant is a deletion, kept by the mate
    that reaches 20 bases past it and dropped by the one that reaches 5."""
    gidx = tail_index(n_var)
    assert n_var % 32 in (0, 1, 31)
    far, near, past = mate(n_var - 40, "60M"), mate(n_var - 40, "45M"), mate(n_var - 30, "30M", [(29, "C")])
    rec = sample([(far, near), (past, far), (near, past)] * 3)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    last = n_var - 1
    d_far, d_near, d_past = want["mates"][:3]
    assert d_far["hi"] == d_near["hi"] == n_var and d_past["hi"] == n_var       # (its last event is novel: right edge n_var)
    assert want["ids"][want["off"][3] - 1] == last                             # left negatives of pair 0 end with the deletion
    assert d_far["n_neg"] == d_near["n_neg"] + 1 == 40
    assert not d_past["events"][0]["known"]


@pytest.mark.parametrize("at_bit_31", [1, 2, 3])
def test_deletions_at_the_right_edge_rule_across_two_kept_words(device, monkeypatch, at_bit_31):
    """KIRA 3000 carries deletions of 1, 2 and 3: pos + length + 10 = right - 1, right, right + 1 for a right edge of 3012.
    Only the first is a negative.  The deletion of ``at_bit_31`` is candidate 31 of the window, the next one candidate 32."""
    gidx = dense_index()
    pos0 = 3000 - 31 + at_bit_31
    target = mate(pos0, f"{3012 - pos0}M")
    rec, ats = around([target, mate(pos0, f"{3013 - pos0}M"), mate(pos0, f"{3011 - pos0}M")])
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    dels = [ordinal(gidx, 0, 3000, 2, n) for n in (1, 2, 3)]
    d = want["mates"][ats[0]]
    assert d["right"] == 3012 and [3000 + n + 10 - d["right"] for n in (1, 2, 3)] == [-1, 0, 1]
    assert dels[at_bit_31 - 1] - d["lo"] == 31 and d["hi"] > dels[2] and not d["any_n"]
    kept = [[v in want["ids"][_neg_slice(want, a)].tolist() for v in dels] for a in ats]
    assert kept == [[True, False, False], [True, True, False], [False, False, False]]


def _neg_slice(want, m):
    """The slice of ``ids`` that holds the negatives of input mate ``m`` (every pair of these samples is valid)."""
    assert want["counts"][0] == want["counts"][1]
    o = want["off"]
    return slice(int(o[4 * (m >> 1) + 2 + (m & 1)]), int(o[4 * (m >> 1) + 3 + (m & 1)]))


@pytest.mark.parametrize("n", [200, 300])
def test_an_n_in_a_long_window(device, monkeypatch, n):
    """A mate that reads N takes the candidate-by-candidate loop: within the saved bits (200) and beyond them (300), where
    the N sits at candidate 270."""
    gidx = dense_index()
    off_n = 50 if n == 200 else 270
    rec, (at,) = around([mate(400, f"{n - 1}M", [(20, "C"), (off_n, "N"), (n - 20, "C")])], filler=known_only)
    want, ran = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at]
    assert d["hi"] - d["lo"] == n and d["any_n"] and d["n_events"] == 3 and d["n_neg"] == n - 3
    assert (400 + off_n) not in want["ids"][_neg_slice(want, at)].tolist()      # below 1500 an ordinal is a position
    assert ran["records"] == (["tab_emit"] if n > 256 else ["tab_expand"])


# ------------------------------------------------------------------------------------------------ bounds and look-ups
def _bounds_cases():
    c = {}
    c["pos0 = 0, event at 0"] = (mate(0, "50M", [(0, "C"), (10, "G")]), lambda d, g: d["lo"] == 0 and d["events"][0]["ordinal"] == 0)
    end_c = lambda d, g: d["hi"] == g.n_variant                                     # noqa: E731
    # right edge at KIRC's last variant position, + 1, + 2, far beyond (11 substitutions, the insertion and the deletion at
    # 192; the deletion reaches within 10 bases of the first three edges)
    for k, s in enumerate((50, 51, 52, 150)):
        c[f"KIRC right edge {150 + s}"] = (mate(150, f"{s}M", ref=2), lambda d, g, s=s: d["right"] == 150 + s and end_c(d, g)
                                           and d["hi"] - d["lo"] == 13 and d["n_neg"] == (13 if s == 150 else 12))
    c["KIRC pos0 200"] = (mate(200, "30M", ref=2), lambda d, g: d["hi"] - d["lo"] == 1 and end_c(d, g))
    for p in (201, 202, 900):
        c[f"KIRC pos0 {p}"] = (mate(p, "30M", [(3, "C")], ref=2), lambda d, g: d["lo"] == d["hi"] == g.n_variant
                               and not d["events"][0]["known"] and d["n_neg"] == 0)
    end_a = lambda d, g: d["hi"] == int(g.gene_vbeg[1])                             # noqa: E731
    c["KIRA right edge 3499"] = (mate(3450, "49M"), lambda d, g: end_a(d, g) and d["hi"] - d["lo"] == 50)
    c["KIRA right edge 3500"] = (mate(3450, "50M"), lambda d, g: end_a(d, g) and d["hi"] - d["lo"] == 50)
    c["KIRA pos0 3499"] = (mate(3499, "30M", [(0, "C")]), lambda d, g: end_a(d, g) and d["hi"] - d["lo"] == 1 and d["events"][0]["known"])
    for p in (3500, 3501, 4000):
        c[f"KIRA pos0 {p}"] = (mate(p, "30M", [(0, "C")]), lambda d, g: d["lo"] == d["hi"] == int(g.gene_vbeg[1])
                               and not d["events"][0]["known"])
    c["KIRB without variants"] = (mate(0, "50M", [(0, "C"), (20, "G")], ref=1), lambda d, g: d["lo"] == d["hi"] == int(g.gene_vbeg[1])
                                  and not any(e["known"] for e in d["events"]) and d["n_pos"] == 2)
    c["KIRB insertion and deletion"] = (mate(40, "10M2I10M3D10M", ins=[0], ref=1), lambda d, g: d["dropped"] and d["n_events"] == 2)
    # substitutions at and beyond the last variant position of KIRC (200)
    c["known substitution at the last position"] = (mate(180, "40M", [(20, "C")], ref=2), lambda d, g: d["events"][0]["ordinal"] == g.n_variant - 1)
    c["novel substitution at the last position"] = (mate(180, "40M", [(20, "G")], ref=2), lambda d, g: not d["events"][0]["known"] and d["n_neg"] == 7)
    c["substitution one past the last position"] = (mate(180, "40M", [(21, "C")], ref=2), lambda d, g: not d["events"][0]["known"] and d["events"][0]["pos"] == 201)
    c["substitution far past the last position"] = (mate(380, "40M", [(20, "C")], ref=2), lambda d, g: not d["events"][0]["known"])
    # insertions and deletions through the bucket table: 15, 16, the last bucket that holds variants (192), the closing one
    # (208 = 16 * 13) and beyond
    for p, ins_known, del_known in ((15, 0, 2), (16, 1, 3), (192, 0, 2)):
        c[f"known insertion at {p}"] = (mate(p - 10, "10M2I30M", ins=[ins_known], ref=2), lambda d, g: d["events"][0]["known"] and d["n_pos"] == 1)
        c[f"novel insertion at {p}"] = (mate(p - 10, "10M2I30M", ins=[ins_known + 2], ref=2), lambda d, g: d["dropped"])
        c[f"known deletion at {p}"] = (mate(p - 10, f"10M{del_known}D30M", ref=2), lambda d, g: d["events"][0]["known"] and d["n_pos"] == 1)
        c[f"novel deletion at {p}"] = (mate(p - 10, f"10M{del_known + 3}D30M", ref=2), lambda d, g: d["dropped"])
    for p in (208, 500):
        c[f"novel insertion at {p}"] = (mate(p - 10, "10M2I30M", ins=[0], ref=2), lambda d, g, p=p: d["dropped"] and d["events"][0]["pos"] == p)
        c[f"novel deletion at {p}"] = (mate(p - 10, "10M2D30M", ref=2), lambda d, g, p=p: d["dropped"] and d["events"][0]["pos"] == p)
    # several variants at one position
    c["insertion and deletion at 120"] = (mate(100, "20M2I2D30M", ins=[0], ref=2), lambda d, g: d["n_pos"] == 2 and
                                          [e["typ"] for e in d["events"]] == [0, 2] and all(e["known"] for e in d["events"]))
    for b in "ACG":
        c[f"insertion and substitution {b} at 120"] = (mate(100, "20M2I30M", [(20, b)], ins=[0], ref=2), lambda d, g: d["n_pos"] == 2 and
                                                       d["events"][1]["ordinal"] == d["events"][0]["ordinal"] + 1 + "ACG".index(
                                                           chr(d["events"][1]["key"] & 0xFF)))
    c["insertion of another string at 100"] = (mate(90, "10M2I30M", ins=[1], ref=2), lambda d, g: d["dropped"])
    c["deletion of another length at 100"] = (mate(90, "10M3D30M", ref=2), lambda d, g: d["dropped"])
    c["known insertion and deletion at 100"] = (mate(90, "10M2I2D30M", ins=[0], ref=2), lambda d, g: d["n_pos"] == 2)
    # the four right-edge forms
    c["right edge: trailing match"] = (mate(600, "50M", [(10, "C")]), lambda d, g: d["right"] == 650 and d["hi"] == 651)
    c["right edge: known last event"] = (mate(600, "50M", [(49, "C")]), lambda d, g: d["right"] == 649 and d["hi"] == 650 and d["n_neg"] == 49)
    c["right edge: novel last substitution"] = (mate(600, "50M", [(49, "G")]), lambda d, g: d["right"] == 650 and d["hi"] == 651 and d["n_neg"] == 51)
    c["right edge: known last insertion"] = (mate(2590, "10M2I", ins=[0]), lambda d, g: d["right"] == 2600 and d["n_pos"] == 1
                                             and d["hi"] == d["events"][0]["ordinal"] + 2)
    return c


BOUNDS = _bounds_cases()


@pytest.mark.parametrize("case", list(BOUNDS))
def test_window_bounds_and_look_ups(device, monkeypatch, case):
    gidx = dense_index()
    assert (200 >> 4) + 1 == 13 and int(gidx.key[-1] >> 32) & 0xFFFFFF == 200      # KIRC: buckets 0 .. 13, the last one at 208
    target, holds = BOUNDS[case]
    rec, (at,) = around([target], n_pairs=12)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at]
    assert d["walked"] and not d["bad_window"] and holds(d, gidx), d
    assert want["pair_gene"][np.searchsorted(want["pair_src"], at >> 1)] == (target["ref"][0] if at % 2 == 0 else 0)


# ------------------------------------------------------------------------------------------------ tab_expand
@pytest.mark.parametrize("n_pairs", [1, 31, 32, 33, 63, 64, 65])
def test_pair_counts_around_a_wave_and_a_workgroup_of_the_expansion(device, monkeypatch, n_pairs):
    gidx = dense_index()
    rec = sample([(ordinary(2 * i), ordinary(2 * i + 1)) for i in range(n_pairs)])
    want, ran = tabulate3(device, monkeypatch, gidx, rec)
    assert want["counts"][1] == n_pairs and ran["records"] == ["tab_expand"]
    assert want["counts"][2] == n_pairs * 2 * (2 + 100)


def _wave(span, first=0):
    """32 pairs of event-free mates of ``span`` bases below 1500: span + 1 ids each."""
    return [(mate(100 + 3 * ((first + 2 * i) % 60), f"{span}M"), mate(110 + 5 * ((first + i) % 60), f"{span}M")) for i in range(32)]


def _wave_ids(want, w):
    o = want["off"]
    assert want["counts"][0] == want["counts"][1]
    return int(o[4 * min(32 * (w + 1), want["counts"][1])]) - int(o[4 * 32 * w])


@pytest.mark.parametrize("run", [4095, 4096, 4097])
def test_a_wave_run_at_the_staging_cap(device, monkeypatch, run):
    """64 mates of 64 ids are 4096; the last mate's span makes the run 4095, 4096 (staged) or 4097 (written directly); the
    waves before and after are staged."""
    gidx = dense_index()
    mid = _wave(63)
    mid[31] = (mid[31][0], mate(700, f"{63 + run - 4096}M"))
    rec = sample(_wave(20) + mid + _wave(20, first=7))
    want, ran = tabulate3(device, monkeypatch, gidx, rec)
    assert [_wave_ids(want, w) for w in range(3)] == [32 * 2 * 21, run, 32 * 2 * 21] and ran["records"] == ["tab_expand"]


def test_a_wave_of_invalid_pairs_between_two_full_ones(device, monkeypatch):
    gidx = dense_index()
    dead = [(mate(300 + i, "50M", [(5, "G")], flag=1), mate(400 + i, "50M", [(6, "A")])) for i in range(32)]
    rec = sample(_wave(40) + dead + _wave(40, first=3))
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    assert want["counts"][1] == 64 and want["pair_src"].tolist() == list(range(32)) + list(range(64, 96))
    assert not any(d["walked"] for d in want["mates"][64:128]) and want["counts"][3] == 0


def test_wide_pairs_inside_a_staged_and_a_direct_wave(device, monkeypatch):
    """Pair 16 (wave 0, staged) and pair 48 (wave 1, more than 4096 ids: written directly) are of the wide format; tab_expand
    leaves their slots to tab_emit_wide."""
    gidx = dense_index()
    pairs = _wave(40) + _wave(70)
    rec = sample(pairs)
    wl = wide_mate(200, "150M", [(3 + 7 * i, "CG"[i % 2]) for i in range(20)])
    wr = wide_mate(230, "150M", [(2 + 6 * i, "GC"[i % 3 == 0]) for i in range(24)])
    spill = spill_of(rec, {16: (wl, wr), 48: (wr, wl)})
    want, ran = tabulate3(device, monkeypatch, gidx, rec, spill=spill)
    assert _wave_ids(want, 0) <= 4096 < _wave_ids(want, 1) and ran["records"] == ["tab_expand"]
    for m in (32, 33, 96, 97):
        assert want["mates"][m]["n_events"] in (20, 24) and want["mates"][m]["n_pos"] > 16 and want["mates"][m]["n_neg"] > 100
    assert want["counts"][3] > 10


def test_an_invalid_pair_and_a_dropped_mate_between_lists(device, monkeypatch):
    gidx = dense_index()
    pairs = _wave(30)
    pairs[10] = (mate(300, "50M", [(5, "G")], nm=5), mate(400, "50M"))                  # NM > 4: the pair goes
    pairs[11] = (mate(300, "20M3D30M", [(5, "G")]), mate(400, "50M", [(7, "G")]))       # novel deletion: the mate yields nothing
    pairs[12] = (mate(300, "5S45M", [(5, "A")]), mate(400, "50M"))                      # clipped
    rec = sample(pairs)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    m = want["mates"]
    assert not m[20]["walked"] and m[22]["dropped"] and m[22]["n_events"] == 2 and m[24]["clipped"] and want["counts"][1] == 31
    assert want["counts"][3] == 3 and m[23]["n_pos"] == 1 and m[23]["n_neg"] == 51


# ------------------------------------------------------------------------------------------------ cooperative enumeration
def _span(n):
    """A mate whose window has exactly n candidates (no event)."""
    return hole() if n == 0 else mate(1590, "10M") if n == 1 else mate(500, f"{n - 1}M")


def test_windows_of_a_wave_laid_end_to_end(device, monkeypatch):
    """tab_emit, 256 mates = 4 waves.  Wave 0: the first owner's window is 63 candidates, the second one's 130 -- it starts
    at candidate 63 of step 0 and ends in step 3 --, then owners with empty windows between non-empty ones.  Wave 1: 64
    candidates in all (one full step), wave 2: 128 (two), wave 3: none."""
    gidx = dense_index()
    w0 = [63, 130] + [0, 10, 0, 0, 33, 1] * 10 + [0, 5]
    w1 = [0] * 20 + [32] + [0] * 30 + [31, 1] + [0] * 11
    w2 = [32, 0, 32, 0] + [0] * 56 + [0, 32, 0, 32]
    w3 = [0] * 64
    lens = w0 + w1 + w2 + w3
    assert [len(w) for w in (w0, w1, w2, w3)] == [64] * 4 and sum(w1) == 64 and sum(w2) == 128
    rec = np.ascontiguousarray(np.concatenate([_span(n) for n in lens]))
    want, ran = tabulate3(device, monkeypatch, gidx, rec)
    got = [d["hi"] - d["lo"] for d in want["mates"]]
    assert got == lens and [d["n_neg"] for d in want["mates"]] == lens
    assert ran["two_walks"] == ["tab_emit"] and ran["records"] == ["tab_expand"]


# ------------------------------------------------------------------------------------------------ novel ranks
def _rank_of(want, key):
    return want["novel_key"].tolist().index(key)


def test_first_appearance_is_not_launch_order(device, monkeypatch):
    """Mate 5 meets the key as its event 3, mate 300 (the second workgroup of pass 1) as its event 0."""
    gidx = dense_index()
    pairs = [(ordinary(2 * i), ordinary(2 * i + 1)) for i in range(160)]
    pairs[2] = (pairs[2][0], mate(900, "100M", [(5, "C"), (10, "C"), (15, "C"), (33, "T")]))
    pairs[150] = (mate(930, "100M", [(3, "T"), (50, "C")]), pairs[150][1])
    rec = sample(pairs)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    a, b = want["mates"][5]["events"][3], want["mates"][300]["events"][0]
    assert a["key"] == b["key"] == makeKey(0, 933, 1, T) and not a["known"]
    r = _rank_of(want, a["key"])
    before = {e["key"] for d in want["mates"][:5] for e in d["events"] if not e["known"]}
    assert r == len(before) and want["counts"][3] > r + 20
    assert want["ids"][want["off"][4 * 2 + 1] + 3] == gidx.n_variant + r == want["ids"][want["off"][4 * 150]]


def test_a_mate_of_22_novel_events(device, monkeypatch):
    gidx = dense_index()
    rec, (at,) = around([_six_ins(_mm(16, novel=range(16)), ins=(10, 11, 12, 13, 14, 15))])
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    d = want["mates"][at]
    keys = [e["key"] for e in d["events"]]
    assert d["n_events"] == 22 and not any(e["known"] for e in d["events"]) and len(set(keys)) == 22 and d["dropped"]
    r0 = _rank_of(want, keys[0])
    assert want["novel_key"].tolist()[r0:r0 + 22] == keys


def test_ids_of_dropped_invalid_and_clipped_mates(device, monkeypatch):
    """A novel deletion in a dropped mate takes an id, and so does the substitution after it; the mates of an invalid pair
    and a clipped mate carry keys of their own that get none."""
    gidx = dense_index()
    pairs = [(known_only(2 * i), known_only(2 * i + 1)) for i in range(24)]
    pairs[4] = (mate(300, "20M3D30M", [(30, "G")]), mate(400, "50M", [(7, "A")]))
    pairs[5] = (mate(600, "50M", [(8, "T")]), known_only(1))
    pairs[6] = (mate(700, "50M", [(5, "A")], flag=1), mate(710, "50M", [(6, "A")]))
    pairs[7] = (mate(720, "50M", [(5, "A")]), mate(730, "50M", [(6, "A")], nm=255))
    pairs[8] = (mate(740, "5S45M", [(5, "A")]), mate(750, "45M5S", [(6, "A")]))
    pairs[9] = (mate(760, "50M", [(9, "A")]), known_only(3))
    rec = sample(pairs)
    want, _ = tabulate3(device, monkeypatch, gidx, rec)
    m = want["mates"]
    assert m[8]["dropped"] and m[16]["clipped"] and m[17]["clipped"] and not m[12]["walked"] and not m[14]["walked"]
    assert want["novel_key"].tolist() == [makeKey(0, 320, 2, 3), makeKey(0, 330, 1, G), makeKey(0, 407, 1, A), makeKey(0, 608, 1, T),
                                          makeKey(0, 769, 1, A)]
    assert want["counts"][1] == 22


def test_a_wide_pair_early_in_the_sample(device, monkeypatch):
    """70 novel events in a wide mate (event bits 31, 32 and beyond 64 of its words); the plain mates after it go on with
    the numbering, one of them with a key the wide mate met first."""
    gidx = dense_index()
    pairs = [(known_only(2 * i), known_only(2 * i + 1)) for i in range(40)]
    pairs[1] = (mate(20, "50M", [(4, "A")]), known_only(0))
    pairs[5] = (mate(100 + 63, "50M", [(0, "G"), (9, "T")]), mate(900, "60M", [(11, "A")]))      # 163 G: event 31 of the wide mate
    rec = sample(pairs)
    wl = wide_mate(100, "200M", [(2 * i + 1, "G") for i in range(70)])
    wr = wide_mate(400, "200M", [(3 * i, "A") for i in range(40)])
    spill = spill_of(rec, {3: (wl, wr)})
    want, _ = tabulate3(device, monkeypatch, gidx, rec, spill=spill)
    d = want["mates"][6]
    assert d["n_events"] == 70 and not any(e["known"] for e in d["events"]) and d["events"][31]["key"] == makeKey(0, 163, 1, G)
    keys = want["novel_key"].tolist()
    assert keys[0] == makeKey(0, 24, 1, A) and keys[1:71] == [e["key"] for e in d["events"]]
    assert keys[71:111] == [e["key"] for e in want["mates"][7]["events"]]
    assert keys[111:] == [makeKey(0, 172, 1, T), makeKey(0, 911, 1, A)] and want["mates"][10]["events"][0]["key"] == keys[32]


def test_probes_that_wrap_in_a_table_of_16_slots(device, monkeypatch):
    """novel_log2cap=4: three keys whose probes start at slot 15 occupy 15, 0 and 1; five more keys fill the table to its
    accepted half.  The lists equal the default-size run and the restatement."""
    gidx = dense_index()
    at15 = [p for p in range(100, 1400) if hash64(makeKey(0, p, 1, G)) & 15 == 15][:3]
    low = [p for p in range(100, 1400) if hash64(makeKey(0, p, 1, G)) & 15 in (0, 1, 2)][:3]
    rest = [p for p in range(100, 1400) if hash64(makeKey(0, p, 1, G)) & 15 in (7, 8)][:2]
    assert len(at15) == 3 and len(low) == 3 and len(rest) == 2
    pairs = [(known_only(2 * i), known_only(2 * i + 1)) for i in range(12)]
    order = [at15[0], low[0], at15[1], rest[0], at15[2], low[1], low[2], rest[1]]
    for j, p in enumerate(order):
        pairs[1 + j] = (mate(p - 20, "60M", [(20, "G")]), mate(order[j - 1] - 10, "60M", [(10, "G")] if j else []))
    rec = sample(pairs)
    small, _ = tabulate3(device, monkeypatch, gidx, rec, hooks="novel_log2cap=4")
    default, _ = tabulate3(device, monkeypatch, gidx, rec, routes=("records",))
    assert small["novel_key"].tolist() == default["novel_key"].tolist() == [makeKey(0, p, 1, G) for p in order]
    assert small["counts"][3] == 8      # 8 keys in 16 slots: accepted without a retry


# ------------------------------------------------------------------------------------------------ correction table
def test_correction_table_at_the_end_of_its_cover(device, monkeypatch):
    """The table covers KIRA [0, 1000), nothing of KIRB, KIRC [0, 50): rows 0 .. 999 and 1000 .. 1049.  An entry at a
    gene's last covered position is applied, a mismatch one past it is left alone (KIRA 1000 would read KIRC's row 0);
    rewrites make a novel base known, a known one novel, and an N a plain base."""
    gidx = dense_index()
    pos0 = np.array([0, 1000, 1000, 1050], dtype=np.int64)
    table = np.zeros((1050, 5), dtype=np.uint8)
    table[500, 2] = C_          # G -> C: novel -> known
    table[510, 1] = A           # C -> A: known -> novel
    table[520, 4] = C_          # N -> C
    table[999, 2] = C_          # the last row of KIRA
    table[1000, 2] = C_         # KIRC 0: must not touch KIRA 1000
    table[1049, 2] = A          # KIRC 49, the last row: G -> A
    table[1045, 2] = C_         # KIRC 45: G -> C, known
    items = [mate(480, "60M", [(20, "G"), (30, "C"), (40, "N")]),
             mate(960, "60M", [(39, "G"), (40, "G")]),
             mate(30, "40M", [(15, "G"), (19, "G"), (20, "G")], ref=2),
             mate(10, "30M", [(5, "G")], ref=1),
             mate(480, "60M", [(21, "G"), (41, "N")])]
    rec, at = around(items, filler=known_only)
    plain, _ = tabulate3(device, monkeypatch, gidx, rec, routes=("records",))
    want, _ = tabulate3(device, monkeypatch, gidx, rec, correction=(table, pos0))
    d = want["mates"][at[0]]
    assert [e["known"] for e in d["events"]] == [True, False, True] and not d["any_n"] and plain["mates"][at[0]]["any_n"]
    assert [e["known"] for e in plain["mates"][at[0]]["events"]] == [False, True, False]
    assert d["events"][1]["key"] == makeKey(0, 510, 1, A) and d["events"][2]["ordinal"] == 520
    d = want["mates"][at[1]]
    assert d["events"][0]["known"] and d["events"][0]["pos"] == 999 and d["events"][1]["key"] == makeKey(0, 1000, 1, G)
    d = want["mates"][at[2]]
    assert d["events"][0]["known"] and [e["key"] for e in d["events"][1:]] == [makeKey(2, 49, 1, A), makeKey(2, 50, 1, G)]
    assert want["mates"][at[3]]["events"][0]["key"] == makeKey(1, 15, 1, G)
    assert want["mates"][at[4]]["any_n"] and want["mates"][at[4]]["events"][1]["is_n"]
