"""CPU restatement of the compatibility kernel (helper of the compatibility tests, not a test), the list-to-CSR packing
the tests share, and the hand-built sample whose rows leave the normal range of a double.

An entry of the table is the ordered product of one factor per kept id of the row, walked in CSR order (lpv, rpv, lnv,
rnv): 0.999 where read and allele agree, 0.001 where they do not.  Multiplying one factor at a time in float64 is what
the reference's ``np.stack(factors).prod(axis=0)`` does (a reduction over the leading axis runs row by row), so the
products below are its bits -- subnormals and ``+0.0`` included.  ``np.prod`` along a row or a pairwise reduce would not
be: their order is another.

Nothing here imports ``oracle/`` or the package's engine."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

HIT, MISS = 0.999, 0.001
MISS_CAP = 100          # a count from here on is stored as 255 in the mismatch table and sends the gene to the exact search
NVAR_CAP = 4096         # so does a row with this many kept ids


def packLists(lists) -> tuple[np.ndarray, np.ndarray]:
    """``lists``: per row ``(lpv, rpv, lnv, rnv)`` of variant ordinals -> (off uint32 [4 n + 1], ids uint32)."""
    off = np.zeros(4 * len(lists) + 1, dtype=np.uint32)
    flat: list[int] = []
    for i, row in enumerate(lists):
        assert len(row) == 4
        for k, lst in enumerate(row):
            flat.extend(int(v) for v in lst)
            off[4 * i + k + 1] = len(flat)
    return off, np.array(flat, dtype=np.uint32)


def packMask(bits: np.ndarray) -> np.ndarray:
    """bool [n_span][n_allele] -> the bit rows uint32 [max(n_span, 1)][ceil(n_allele / 32)] (bit a & 31 of word a >> 5)."""
    bits = np.asarray(bits, dtype=bool)
    n_span, n_allele = bits.shape
    words = max((n_allele + 31) // 32, 1)
    padded = np.zeros((max(n_span, 1), 32 * words), dtype=np.uint8)
    padded[:n_span, :n_allele] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32)


class CompatRef(NamedTuple):
    probs: np.ndarray       # float64 [n_rows][n_allele]
    miss: np.ndarray        # int64   [n_rows][n_allele]: exact mismatch counts
    nvar: np.ndarray        # int64   [n_rows]: kept ids
    log: np.ndarray         # float64 [n_rows][n_allele]: numpy.log10(probs)

    @property
    def miss_u8(self) -> np.ndarray:
        """The counts of the product path (``gk_compat``): saturated at 255."""
        return np.minimum(self.miss, 255).astype(np.uint8)

    @property
    def miss8(self) -> np.ndarray:
        """The bytes of the mismatch table (``gk_compat_log_miss``): the count below 100, else 255."""
        return np.where(self.miss < MISS_CAP, self.miss, 255).astype(np.uint8)

    @property
    def flag0(self) -> bool:
        """Bit 0 of the flag word: some count >= 100 or some row of >= 4096 kept ids."""
        return bool((self.miss >= MISS_CAP).any() or (self.nvar >= NVAR_CAP).any())


def compatReference(off, ids, rows, vflag, vbeg: int, vend: int, bits, keep_empty: bool) -> CompatRef:
    """``bits``: bool [vend - vbeg][n_allele], the gene's bit rows.  No allele carries an id outside [vbeg, vend)."""
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    vflag = np.asarray(vflag, dtype=np.uint8)
    bits = np.asarray(bits, dtype=bool).reshape(vend - vbeg, -1)
    n_allele = bits.shape[1]
    nobody = np.zeros(n_allele, dtype=bool)
    probs = np.empty((len(rows), n_allele), dtype=np.float64)
    miss = np.zeros((len(rows), n_allele), dtype=np.int64)
    nvar = np.zeros(len(rows), dtype=np.int64)
    for i, r in enumerate(rows):
        r = int(r)
        b, mid, e = off[4 * r], off[4 * r + 2], off[4 * r + 4]
        p = np.ones(n_allele, dtype=np.float64)
        for k in range(b, e):
            v = int(ids[k])
            positive = k < mid
            if vflag[v] & (1 if positive else 2):
                continue
            carries = bits[v - vbeg] if vbeg <= v < vend else nobody
            agree = carries if positive else ~carries
            p = p * np.where(agree, HIT, MISS)
            miss[i] += ~agree
            nvar[i] += 1
        probs[i] = p if nvar[i] else (HIT if keep_empty else 1.0)
    with np.errstate(divide="ignore"):
        log = np.log10(probs)
    return CompatRef(probs, miss, nvar, log)


def tally(off, ids, rows, vflag, n_var_total: int) -> tuple[np.ndarray, np.ndarray]:
    """(positive, negative) counts per ordinal of the ids of ``rows`` that survive ``vflag``."""
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    vflag = np.asarray(vflag, dtype=np.uint8)
    pos, neg = [], []
    for r in rows:
        r = int(r)
        p, q = ids[off[4 * r]:off[4 * r + 2]], ids[off[4 * r + 2]:off[4 * r + 4]]
        pos.append(p[(vflag[p] & 1) == 0])
        neg.append(q[(vflag[q] & 2) == 0])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
    return (np.bincount(cat(pos), minlength=n_var_total).astype(np.uint32),
            np.bincount(cat(neg), minlength=n_var_total).astype(np.uint32))


def correctionFlags(pos, neg) -> np.ndarray:
    """Drop flags of one error-correction pass over the tallies: bit 0 = out of the positive lists, bit 1 = out of the
    negative ones (fewer than 3 observations: both; a side below a fifth of them: that side)."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    n = pos + neg
    flags = np.zeros(len(n), dtype=np.uint8)
    seen = n > 0
    few = seen & (n < 3)
    flags[few] = 3
    rest = seen & ~few
    with np.errstate(divide="ignore", invalid="ignore"):
        flags[rest & (pos / n < 0.2)] |= 1
        flags[rest & (neg / n < 0.2)] |= 2
    return flags


# ---------------------------------------------------------------------------------------------------------------------
# The hand-built sample that enters the underflow regime.
#
# Two genes of SNP sites three bases apart.  Allele 0 of a gene carries six sites in ten; every other allele is allele 0
# with a chosen NUMBER of sites flipped inside each of three windows of 330 sites, so a long read of allele 0 over a
# window (two mates of 165 sites) mismatches that allele exactly that often.  Where the flipped sites lie in the row's
# list order differs per window: at the head of the list, at its tail, spread evenly -- the roundings of the subnormal
# products depend on it.  The heavy gene's counts cross 100 (the mismatch byte saturates), 103 - 107 (subnormal
# products) and 108 (the product is +0.0, its log10 -inf); the companion gene stops at 99.  ~300 short pairs of alleles 0
# and 1, laid out at a fixed step, give every site enough observations on both sides to pass the error correction
# untouched.  Sample "b" adds three identical reads over a fourth window whose sites every allele carries and the reads
# do not: rows that underflow for EVERY allele, so every set of the heavy gene scores -inf.
HEAVY_COUNTS = [0, 30, 60, 90, 98, 99, 100, 101, 102, 103, 107, 108, 109, 120, 254, 255, 256, 300]
CAPPED_COUNTS = [0, 30, 60, 90, 98, 99]
# sorted, the heavy gene's variants start above 0; both names are of genes the drivers never type as homozygous, so every
# copy-number step is searched
HEAVY_GENE, CAPPED_GENE = "KIR2DL5*BACKBONE", "KIR2DL1S1*BACKBONE"
PLACEMENTS = ("first", "last", "interleaved")
_STEP, _HALF, _GAP = 3, 165, 30              # bases between sites, sites per mate, bases without a site between the mates
_WINDOW0, _WINDOW_PITCH = 300, 1100          # first site of window 0, distance between windows
_KILL0, _KILL_HALF = 3900, 65                # the window every allele carries: first site, sites per mate
_LENGTH = 4500


def _windowSites(w0: int, half: int) -> tuple[list[int], list[int]]:
    lo = [w0 + _STEP * j for j in range(half)]
    start_hi = lo[-1] + _STEP + _GAP
    return lo, [start_hi + _STEP * j for j in range(half)]


def _flipped(placement: str, n_slots: int, m: int) -> set[int]:
    """List positions (0 = the row's first factor) of the ``m`` factors that mismatch."""
    if placement == "first":
        return set(range(m))
    if placement == "last":
        return set(range(n_slots - m, n_slots))
    return {(i * n_slots) // m for i in range(m)} if m else set()


def underflowIndex():
    """(SynthIndex of the two genes, {gene: [per window: the site positions in the ROW's list order]})."""
    from kir_graph_amd.msa2hisat import Variant
    from kir_graph_amd.synth import BASES, SynthIndex
    rng = np.random.default_rng(1408)
    genes = sorted([HEAVY_GENE, CAPPED_GENE])
    backbone, exons, alleles, variants, order = {}, {}, {}, [], {}
    for g in genes:
        counts = HEAVY_COUNTS if g == HEAVY_GENE else CAPPED_COUNTS
        seq = BASES[rng.integers(0, 4, _LENGTH)]
        backbone[g] = seq
        names = [f"{g.split('*')[0]}*{k + 1:03d}0101" for k in range(len(counts))]
        alleles[g] = names
        carried: dict[int, set[int]] = {}          # site -> alleles (by number) that carry it
        order[g] = []
        for w, placement in enumerate(PLACEMENTS):
            lo, hi = _windowSites(_WINDOW0 + _WINDOW_PITCH * w, _HALF)
            sites = lo + hi
            base = {p: (7 * j) % 10 < 6 for j, p in enumerate(sites)}          # allele 0
            # the row of a read of allele 0: its alt bases (positives) of the left mate, of the right mate, then the
            # sites it shows the reference base at (negatives), left and right
            listed = [p for p in lo if base[p]] + [p for p in hi if base[p]] + \
                     [p for p in lo if not base[p]] + [p for p in hi if not base[p]]
            order[g].append(listed)
            for a, m in enumerate(counts):
                flips = {listed[t] for t in _flipped(placement, len(listed), m)}
                for p in sites:
                    if base[p] != (p in flips):
                        carried.setdefault(p, set()).add(a)
                    else:
                        carried.setdefault(p, set())
        lo, hi = _windowSites(_KILL0, _KILL_HALF)
        for p in lo + hi:
            carried[p] = set(range(len(counts)))
        order[g].append(lo + hi)
        exons[g] = [(330, 480), (1500, 1560), (2700, 2790)]
        for p in sorted(carried):
            if not carried[p]:
                continue            # a site nobody carries is no variant of the index
            alt = chr(int(BASES[(int(np.searchsorted(BASES, seq[p])) + 1) % 4]))
            variants.append(Variant(pos=p, typ="single", ref=g, val=alt, length=1,
                                    allele=sorted(names[a] for a in carried[p]),
                                    in_exon=any(s <= p < e for s, e in exons[g])))
    variants.sort()
    for i, v in enumerate(variants):
        v.id = f"hv{i}"
    return SynthIndex(genes=genes, backbone=backbone, variants=variants, exons=exons, alleles=alleles), order


def _mate(bb: np.ndarray, start: int, length: int, alt: dict[int, str]) -> tuple[str, str, str]:
    """(CIGAR, MD, SEQ) of ``length`` bases from ``start`` that show ``alt[p]`` at the positions of ``alt``."""
    seq = list(bb[start:start + length].tobytes().decode())
    md, last = "", start
    for p in sorted(p for p in alt if start <= p < start + length):
        md += f"{p - last}{seq[p - start]}"
        seq[p - start] = alt[p]
        last = p + 1
    return f"{length}M", md + str(start + length - last), "".join(seq)


def _pairLines(name: str, gene: str, bb: np.ndarray, alt: dict[int, str], lo: tuple[int, int], hi: tuple[int, int]) -> list[str]:
    recs = [(s, *_mate(bb, s, n, alt)) for s, n in (lo, hi)]
    lines = []
    for t, flag in ((1, 99), (0, 147)):      # the lower mate is the LATER line: the left lists of the row are its ids
        start, cigar, md, seq = recs[t]
        lines.append("\t".join([name, str(flag), gene, str(start + 1), "60", cigar, "=", str(recs[1 - t][0] + 1), "0", seq,
                                "I" * len(seq), "AS:i:0", "ZS:i:0", "XN:i:0", "NM:i:0", f"MD:Z:{md}", "YS:i:0", "YT:Z:CP",
                                "NH:i:1"]))
    return lines


def underflowLines(sidx, which: str) -> list[str]:
    """SAM lines of sample ``"a"`` (long reads of allele 0 over the three windows of both genes + the short pairs) or
    ``"b"`` (the same + three reads over the fourth window of the heavy gene that mismatch every allele 130 times)."""
    assert which in ("a", "b")
    lines, n = [], 0
    for g in sidx.genes:
        bb = sidx.backbone[g]
        names = sidx.alleles[g]
        alt_of = [{v.pos: str(v.val) for v in sidx.variants if v.ref == g and names[a] in v.allele} for a in (0, 1)]
        for w in range(len(PLACEMENTS)):
            lo, hi = _windowSites(_WINDOW0 + _WINDOW_PITCH * w, _HALF)
            span = _STEP * (_HALF - 1) + 3
            lines += _pairLines(f"heavy{n:04d}", g, bb, alt_of[0], (lo[0] - 1, span), (hi[0] - 1, span))
            n += 1
        for i in range(300):
            u = 250 + 11 * i
            lines += _pairLines(f"short{n:04d}", g, bb, alt_of[i & 1], (u, 60), (u + 150, 60))
            n += 1
        if which == "b" and g == HEAVY_GENE:
            lo, hi = _windowSites(_KILL0, _KILL_HALF)
            span = _STEP * (_KILL_HALF - 1) + 3
            for _ in range(3):
                lines += _pairLines(f"under{n:04d}", g, bb, {}, (lo[0] - 1, span), (hi[0] - 1, span))
                n += 1
    return lines


# ---------------------------------------------------------------------------------------------------------------------
# Fixture T14 (tests/golden/t14_underflow.json.gz: the reference's own typing of the two samples), shared by the oracle's and
# the HIP path's golden tests.
def _unhex(xs):
    return np.array([float.fromhex(x) for x in xs])


def check_t14_steps(got_steps, want_steps, names_of):
    """Every copy-number step against fixture T14: -inf exactly where the reference has it and no NaN, finite values
    within 1e-9; per-allele sums, abundances, ids and names wherever the reference's value is not tied with another row
    (which of the tied sets holds which rank is numpy's argsort tie order, which depends on the host's SIMD level)."""
    assert len(got_steps) == len(want_steps)
    for got, want in zip(got_steps, want_steps):
        assert got.n == want["n"]
        v = _unhex(want["value"])
        value = np.asarray(got.value, dtype=np.float64)
        assert value.shape == v.shape and not np.isnan(value).any()
        assert np.array_equal(np.isneginf(value), np.isneginf(v))
        assert np.allclose(value, v, rtol=1e-9, atol=0)
        untied = np.array([np.count_nonzero(v == x) == 1 for x in v], dtype=bool)
        for f in ("value_sum_indv", "fraction"):
            x, w = np.asarray(getattr(got, f), dtype=np.float64).reshape(len(v), -1), _unhex(want[f]).reshape(len(v), -1)
            assert x.shape == w.shape and not np.isnan(x).any(), f
            assert np.array_equal(np.isneginf(x[untied]), np.isneginf(w[untied])), f
            assert np.allclose(x[untied], w[untied], rtol=1e-9, atol=0), f
        ids, want_ids = np.asarray(got.allele_id).reshape(len(v), -1), np.asarray(want["allele_id"]).reshape(len(v), -1)
        assert np.array_equal(ids[untied], want_ids[untied])
        names = names_of(got)
        for k in np.flatnonzero(untied):
            assert list(names[k]) == want["allele_name"][k]


def check_t14_calls(calls, want, cn):
    """The calls gene by gene: equal where the reference's best value is not tied; a tied gene still gets cn names."""
    at = 0
    for gene, n in cn.items():
        last = want["genes"][gene][-1]
        v = _unhex(last["value"])
        if np.count_nonzero(v == v[0]) == 1:
            assert calls[at:at + n] == want["calls"][at:at + n], gene
        else:
            assert len(calls[at:at + n]) == n and all(c.startswith(gene.split("*")[0] + "*") for c in calls[at:at + n]), gene
        at += n
    assert at == len(calls) == len(want["calls"])

