"""A plain restatement of the read -> variant-list tabulation on packed RECORDS (``MATE_DTYPE`` / ``MATE_WIDE_DTYPE``).

TEST INFRASTRUCTURE.  ``oracle/tabulate.py`` reads SAM text; a case that has to sit exactly on a limit of the record
format (a fifth event, a 129th candidate, a seventh mismatch) is built as a record, so this module states the same rules
-- the ones ``csrc/gk_tabulate.hip`` cites in its header -- on the fields a record carries:

* filterRead (hisat2.py:541-578): both mates of a pair have flag & 2 and an NM that is present and <= 4;
* recordToRawVariant (279-515): the CIGAR operations are walked with the mismatches of the M runs: match segments,
  substitutions (length 1), insertions and deletions (their length); a soft clip anywhere makes the mate yield nothing
  before any id is assigned (recordToVariants 681-684);
* errorCorrection (609-654) as the per-position table the library takes (``pileup.correctionTable``): a substitution's
  base is replaced by the table's entry where the table covers the position;
* findVariantId (581-606): a variant of the index is found by (ref, pos, typ, val); anything else gets the next id of one
  sequential counter -- pairs in order, the left mate then the right one, events in walk order, a pair of the wide format
  walked in its place -- and is known from then on;
* recordToVariants sorts the mate's variants (689); getVariantsBoundary (692-713) bisects the sorted index with
  (pos of the first, single, 'A') and (pos + length of the last, single, 'T'): index records carry length 0 (readVariants
  159-180 sets none), walker-made ones their own;
* getPNFromVariantList (716-800): a novel insertion or deletion empties both lists of the mate; the positives are the
  non-match variants; the negatives are the window's variants one by one, minus the positives, minus A/C/G/T at a position
  the read calls N, minus deletions with pos + length + 10 >= right edge;
* extractVariant (803-844): lists in the order lpv, rpv, lnv, rnv; NH and backbone of the left record.

Nothing here is a look-up structure of the kernel: a sorted Python list and ``bisect``, a dictionary of novel keys in
order of appearance, a loop over candidates.  ``hash64`` restates the kernel's hash only so that a test can CHOOSE keys
by their first slot; no result depends on it.
"""
from __future__ import annotations

import bisect

import numpy as np

CIG_M, CIG_I, CIG_D, CIG_S = 0, 1, 2, 4                      # include/graphkir_hip.h
NM_ABSENT, SPILLED = 255, 0xFF
TYP_INS, TYP_SINGLE, TYP_DEL, TYP_MATCH = 0, 1, 2, 3         # msa2hisat.TYPE_RANK
CAPS = {"plain": (14, 16, 6, 22), "wide": (128, 256, 120, 384)}      # CIGAR ops, mismatches, strings, events
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("N"): 4}
M64 = (1 << 64) - 1


class CapacityError(ValueError):
    """A filter-passing mate carries more events than its record format holds (the library: GK_ERR_CAPACITY)."""


def makeKey(ref: int, pos: int, typ: int, val: int) -> int:
    return (ref << 56) | (pos << 32) | (typ << 30) | val


def keyFields(k: int) -> tuple[int, int, int, int]:
    return k >> 56, (k >> 32) & 0xFFFFFF, (k >> 30) & 3, k & ((1 << 30) - 1)


def hash64(k: int) -> int:
    """The slot hash of the kernel's novel table (before the mask), for choosing keys only."""
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M64      # noqa: E702
    k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M64      # noqa: E702
    return (k ^ (k >> 33)) & 0xFFFFFFFF


def _fields(r, wide: bool):
    """(ops [(op, len)], mismatches [(ref_off, base)], string ids) of a record."""
    n_cig, n_mm = int(r["n_cig"]), int(r["n_mm"])
    ops = [(int(c) & 15, int(c) >> 4) for c in r["cig"][:n_cig]]
    if wide:
        mms = [(int(x) >> 8, int(x) & 0xFF) for x in r["mm"][:n_mm]]
    else:
        mms = [(int(x["ref_off"]), int(x["base"])) for x in r["mm"][:n_mm]]
    return ops, mms, [int(x) for x in r["ins"]]


def _passes(r) -> bool:
    return bool(int(r["flag"]) & 2) and int(r["nm"]) != NM_ABSENT and int(r["nm"]) <= 4


def _rawVariants(r, wide: bool):
    """recordToRawVariant on a record: [(pos, typ, val, length)] with the match segments, or None when clipped."""
    cap_cig, cap_mm, cap_ins, _ = CAPS["wide" if wide else "plain"]
    if int(r["n_cig"]) > cap_cig or int(r["n_mm"]) > cap_mm:
        raise ValueError("the record names more operations or mismatches than its format holds")
    ops, mms, ins = _fields(r, wide)
    if not ops:
        raise ValueError("a mate without CIGAR operations is no record of an alignment")
    if any(op == CIG_S for op, _ in ops):
        return None
    pos0 = int(r["pos0"])
    cur, mi, ii = pos0, 0, 0
    out = []
    for op, n in ops:
        if op == CIG_M:
            end, seg = cur + n, cur
            while mi < len(mms) and pos0 + mms[mi][0] < end:
                p = pos0 + mms[mi][0]
                if p < seg:
                    raise ValueError("a mismatch lies outside the M runs, or the mismatches are not ascending")
                if p > seg:
                    out.append((seg, TYP_MATCH, None, p - seg))
                out.append((p, TYP_SINGLE, mms[mi][1], 1))
                seg = p + 1
                mi += 1
            if seg < end:
                out.append((seg, TYP_MATCH, None, end - seg))
            cur = end
        elif op == CIG_I:
            out.append((cur, TYP_INS, ins[ii] if ii < cap_ins else 0, n))
            ii += 1
        elif op == CIG_D:
            out.append((cur, TYP_DEL, n, n))
            cur += n
        else:
            raise NotImplementedError(f"CIGAR operation {op}")
    if mi != len(mms):
        raise ValueError("mismatches beyond the last M run")
    return out


def tabulateRecords(rec, index, spill=None, correction=None) -> dict:
    """The tabulation of ``rec`` (two records per pair, left first) against ``index`` (a ``GkIndex``).

    ``spill``: (wide records, two per pair; the pairs they stand for, ascending).  ``correction``: (uint8 table
    [positions][5], int64 first table row of every gene [genes + 1]).  Returns ``counts`` = [n_pairs, n_valid, n_ids,
    n_novel, err_flags], ``off``, ``ids``, ``pair_src``, ``pair_gene``, ``pair_nh``, ``novel_key`` as a device tabulation
    exposes them, and ``mates``: per input mate a dictionary of diagnostics (``walked``, ``clipped``, ``dropped``,
    ``bad_window``, ``n_events``, ``events`` = [{"known", "ordinal" | "key", "is_n"}], ``lo``, ``hi``, ``right``,
    ``any_n``, ``n_pos``, ``n_neg``)."""
    keys = [int(k) for k in index.key]
    assert keys == sorted(keys)
    n_var, n_gene = len(keys), len(index.genes)
    n_pairs = len(rec) // 2
    wide_of = {}
    if spill is not None:
        for k, p in enumerate(spill[1]):
            wide_of[int(p)] = (spill[0][2 * k], spill[0][2 * k + 1])
    table = pos0_of = None
    if correction is not None:
        table, pos0_of = correction
    novel: dict[int, int] = {}             # key -> id, in order of first appearance
    err_flags = 0
    off, ids, pair_src, pair_gene, pair_nh, mates = [0], [], [], [], [], []

    def walk(r, wide: bool) -> dict:
        """One mate of a kept pair: its diagnostics, with ``pos`` / ``neg`` lists of ordinals."""
        nonlocal err_flags
        d = {"walked": True, "clipped": False, "dropped": False, "bad_window": False, "n_events": 0, "events": [],
             "lo": 0, "hi": 0, "right": 0, "any_n": False, "pos": [], "neg": []}
        raw = _rawVariants(r, wide)
        if raw is None:
            d["clipped"] = True
            return d
        ref = int(r["ref"])
        if sum(1 for v in raw if v[1] != TYP_MATCH) > CAPS["wide" if wide else "plain"][3]:
            raise CapacityError("a filter-passing mate carries more variant events than its record format allows")
        found = []                         # (pos, typ, val, length as getVariantsBoundary sees it, ordinal or None, key)
        for pos, typ, val, length in raw:
            if typ == TYP_MATCH:
                found.append((pos, typ, None, length, None, None))
                continue
            if typ == TYP_SINGLE and table is not None and ref < n_gene and val in _CODE:
                at = int(pos0_of[ref]) + pos
                if at < int(pos0_of[ref + 1]) and int(table[at, _CODE[val]]):
                    val = int(table[at, _CODE[val]])
            k = makeKey(ref, pos, typ, val)
            i = bisect.bisect_left(keys, k)
            known = i < n_var and keys[i] == k
            if known:
                length = 0                 # the index's own record
            elif k not in novel:
                novel[k] = len(novel)
            is_n = typ == TYP_SINGLE and val == ord("N")
            d["events"].append({"known": known, "ordinal": i if known else None, "key": k, "is_n": is_n, "typ": typ,
                                "pos": pos})
            found.append((pos, typ, val, length, i if known else n_var + novel[k], k))
        d["n_events"] = len(d["events"])
        order = [(v[0], v[1]) for v in found]
        if len(set(order)) != len(order):
            raise ValueError("two variants of one mate share (position, type): their order needs the strings")
        found.sort(key=lambda v: (v[0], v[1]))
        d["right"] = right = found[-1][0] + found[-1][3]
        d["lo"] = lo = bisect.bisect_left(keys, makeKey(ref, found[0][0], TYP_SINGLE, ord("A")))
        d["hi"] = hi = bisect.bisect_left(keys, makeKey(ref, right, TYP_SINGLE, ord("T")))
        d["any_n"] = any(e["is_n"] for e in d["events"])
        if lo > hi:
            d["bad_window"] = True
            err_flags |= 1
            return d
        if any(not e["known"] and e["typ"] != TYP_SINGLE for e in d["events"]):
            d["dropped"] = True
            return d
        d["pos"] = [v[4] for v in found if v[1] != TYP_MATCH]
        mine = set(d["pos"])
        n_at = {v[0] for v in found if v[1] == TYP_SINGLE and v[2] == ord("N")}
        for i in range(lo, hi):
            _, pos, typ, val = keyFields(keys[i])
            if i in mine:
                continue
            if typ == TYP_SINGLE and pos in n_at and val in (ord("A"), ord("C"), ord("G"), ord("T")):
                continue
            if typ == TYP_DEL and pos + val + 10 >= right:
                continue
            d["neg"].append(i)
        return d

    for p in range(n_pairs):
        heads = (rec[2 * p], rec[2 * p + 1])
        is_wide = int(heads[0]["n_cig"]) == SPILLED or int(heads[1]["n_cig"]) == SPILLED
        if is_wide:
            if p not in wide_of or not all(int(h["n_cig"]) == SPILLED for h in heads):
                raise ValueError(f"pair {p} is marked wide but has no wide records")
        pair = wide_of[p] if is_wide else heads
        if not (_passes(pair[0]) and _passes(pair[1])):
            mates += [{"walked": False}, {"walked": False}]
            continue
        left, right = walk(pair[0], is_wide), walk(pair[1], is_wide)
        for d in (left, right):
            d["n_pos"], d["n_neg"] = len(d["pos"]), len(d["neg"])
        mates += [left, right]
        for lst in (left["pos"], right["pos"], left["neg"], right["neg"]):
            ids += lst
            off.append(len(ids))
        pair_src.append(p)
        pair_gene.append(int(heads[0]["ref"]))
        pair_nh.append(int(heads[0]["nh"]))
    return {"counts": np.array([n_pairs, len(pair_src), len(ids), len(novel), err_flags]),
            "off": np.array(off, dtype=np.uint32), "ids": np.array(ids, dtype=np.uint32),
            "pair_src": np.array(pair_src, dtype=np.int32), "pair_gene": np.array(pair_gene, dtype=np.uint8),
            "pair_nh": np.array(pair_nh, dtype=np.uint8), "novel_key": np.array(list(novel), dtype=np.uint64),
            "mates": mates}
