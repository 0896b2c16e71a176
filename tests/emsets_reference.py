"""CPU restatement of the EM strategy's candidate sets (helper of the candidate-set tests, not a test), and the hand-built
genes and row families those tests share.

The rule (typing_em.py:68-104, stated at the top of csrc/gk_em.hip):

* a mate's set is the intersection of the allele rows of its positive ids minus the union of the rows of its negative ids;
  it is empty when the mate has no positive id;
* an id outside ``[vbeg, vend)`` -- another gene's, or a novel ordinal -- has no allele: as a positive it empties the mate,
  as a negative it does nothing;
* the pair's set is ``L & R`` when that is non-empty, else ``L | R``.

Numpy bool arrays only: no GPU, no ctypes, nothing of ``oracle/`` or of the package."""
from __future__ import annotations

import numpy as np


# ------------------------------------------------------------------------------------------------------------ the rule
def candidateSets(off, ids, rows, vbeg: int, vend: int, bits) -> np.ndarray:
    """bool [len(rows)][n_allele].  ``off`` / ``ids``: the CSR (four lists per row: lpv, rpv, lnv, rnv); ``bits``: bool
    [vend - vbeg][n_allele], the gene's allele rows."""
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    bits = np.asarray(bits, dtype=bool)
    bits = bits.reshape(vend - vbeg, bits.shape[-1] if bits.ndim == 2 else -1)
    n_allele = bits.shape[1]
    out = np.zeros((len(rows), n_allele), dtype=bool)

    def mate(pos, neg):
        if len(pos) == 0:
            return np.zeros(n_allele, dtype=bool)
        s = np.ones(n_allele, dtype=bool)
        for v in pos:
            s &= bits[v - vbeg] if vbeg <= v < vend else False
        for v in neg:
            if vbeg <= v < vend:
                s &= ~bits[v - vbeg]
        return s

    for i, r in enumerate(rows):
        o = off[4 * int(r):4 * int(r) + 5]
        left = mate(ids[o[0]:o[1]], ids[o[2]:o[3]])
        right = mate(ids[o[1]:o[2]], ids[o[3]:o[4]])
        both = left & right
        out[i] = both if both.any() else left | right
    return out


def pack(boolsets, words: int) -> np.ndarray:
    """bool [n][n_allele] -> uint32 [n][words], allele a at bit a & 31 of word a >> 5."""
    boolsets = np.asarray(boolsets, dtype=bool)
    n, n_allele = boolsets.shape
    assert n_allele <= 32 * words
    padded = np.zeros((n, 32 * words), dtype=np.uint8)
    padded[:, :n_allele] = boolsets
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32).reshape(n, words)


def sortedRows(packed) -> np.ndarray:
    """The order that puts the rows ascending, word 0 first."""
    packed = np.asarray(packed, dtype=np.uint32)
    return np.lexsort(packed.T[::-1]) if len(packed) else np.zeros(0, dtype=np.int64)


def distinct(packed) -> tuple[np.ndarray, np.ndarray]:
    """(distinct rows ascending, word 0 first; how often each occurs)."""
    packed = np.asarray(packed, dtype=np.uint32)
    if len(packed) == 0:
        return packed.reshape(0, packed.shape[1]), np.zeros(0, dtype=np.int64)
    s = packed[sortedRows(packed)]
    first = np.concatenate([[True], (s[1:] != s[:-1]).any(axis=1)])
    start = np.nonzero(first)[0]
    return np.ascontiguousarray(s[start]), np.diff(np.concatenate([start, [len(s)]])).astype(np.int64)


def packLists(lists) -> tuple[np.ndarray, np.ndarray]:
    """``lists``: per row ``(lpv, rpv, lnv, rnv)`` -> (off uint32 [4 n + 1], ids uint32)."""
    lens = np.array([len(lst) for row in lists for lst in row], dtype=np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    flat = [v for row in lists for lst in row for v in lst]
    return off, np.array(flat, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------------------ genes
def lanesOf(words: int) -> int:
    """Lanes per pair of the candidate-set kernel (two words per lane): ids are handed round 4 G at a time."""
    return 2 if words <= 4 else 4 if words <= 8 else 8


class Gene:
    """A hand-built gene over the variants ``[vbeg, vend)`` of a universe of ``n_var`` indexed and ``n_total - n_var``
    novel ordinals.  Its allele rows, by name (``self.at``: name -> ordinal):

    * ``all`` (the gene's first variant), ``none``;
    * ``only j`` -- allele j alone, for every j: bit 0 and bit 31 of every word, the first and the last allele, both
      sides of every word boundary;
    * ``but j`` -- every allele except j;
    * ``pairL w`` / ``pairR w`` -- two rows that share one allele of word w and nothing else, their other alleles in
      two other words (for w the first, a middle and the last word);
    * ``fav k`` -- 64 sparse rows, each with allele 3 (six in ten) or allele 7: reads of these favour two alleles;
    * ``filler`` rows in the middle of the span (random halves) up to the wanted ``n_span``;
    * ``rnd k`` -- 40 random halves, the last of them the gene's last variant."""

    N_FAV, N_RND = 64, 40

    def __init__(self, words: int, n_allele: int, n_span: int | None = None, vbeg: int = 37, n_var: int | None = None,
                 n_total: int | None = None, seed: int = 0):
        assert 8 <= n_allele and 32 * (words - 1) < n_allele <= 32 * words
        rng = np.random.default_rng(1000 * words + n_allele + seed)
        self.words, self.n_allele, self.vbeg, self.G = words, n_allele, vbeg, lanesOf(words)
        rows, self.at = [], {}

        def add(name, row):
            self.at[name] = vbeg + len(rows)
            rows.append(np.asarray(row, dtype=bool))

        every, eye = np.ones(n_allele, dtype=bool), np.eye(n_allele, dtype=bool)
        add("all", every)
        add("none", ~every)
        for j in range(n_allele):
            add(("only", j), eye[j])
        for j in range(n_allele):
            add(("but", j), ~eye[j])
        self.pair_words = sorted({0, words // 2, words - 1})
        for w in self.pair_words:
            lo, hi = 32 * w, min(32 * w + 32, n_allele)
            shared = lo + (hi - lo) // 2
            if words > 2:
                x_l, x_r = 32 * ((w + 1) % words) + 1, 32 * ((w + 2) % words) + 2
            else:      # one or two words: the other alleles wherever there is room
                x_l, x_r = (shared + 1) % n_allele, (shared + 2) % n_allele
            assert len({shared, x_l, x_r}) == 3 and max(x_l, x_r) < n_allele
            add(("pairL", w), eye[shared] | eye[x_l])
            add(("pairR", w), eye[shared] | eye[x_r])
        for k in range(self.N_FAV):
            row = rng.random(n_allele) < 0.15
            row[[3, 7]] = False
            row[3 if rng.random() < 0.6 else 7] = True
            add(("fav", k), row)
        n_front = len(rows)
        n_span = n_front + self.N_RND if n_span is None else n_span
        n_fill = n_span - n_front - self.N_RND
        assert n_fill >= 0, (n_span, n_front)
        self.filler = vbeg + n_front + np.arange(n_fill)
        self.rnd = vbeg + n_front + n_fill + np.arange(self.N_RND)
        self.bits = np.concatenate([np.array(rows), rng.random((n_fill + self.N_RND, n_allele)) < 0.5])
        self.bits.setflags(write=False)
        self.n_span, self.vend = n_span, vbeg + n_span
        self.n_var = self.vend + 63 if n_var is None else n_var
        self.n_total = self.n_var + 40 if n_total is None else n_total
        assert self.vend <= self.n_var <= self.n_total
        self.mask = pack(self.bits, words)

    # ids that are not the gene's: other genes' on both sides, novel ordinals
    @property
    def below(self):
        return np.arange(0, self.vbeg)

    @property
    def above(self):
        return np.arange(self.vend, self.n_var)

    @property
    def novel(self):
        return np.arange(self.n_var, self.n_total)


def lengths(G: int) -> list[int]:
    return [0, 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G - 1, 8 * G, 8 * G + 1, 100]


def rowFamilies(g: Gene, seed: int = 0) -> list[tuple[str, list[list[int]], bool]]:
    """The pairs every case is made of: (what it is for, [lpv, rpv, lnv, rnv], names an id of another gene?)."""
    rng = np.random.default_rng(77 + g.words + seed)
    at, n_allele = g.at, g.n_allele
    A, NONE = at["all"], at["none"]
    fams: list[tuple[str, list[list[int]], bool]] = []

    def fam(name, lpv=(), rpv=(), lnv=(), rnv=(), foreign=False):
        fams.append((name, [[int(v) for v in lst] for lst in (lpv, rpv, lnv, rnv)], foreign))

    # ---- list lengths: every position of a list takes one allele away (a positive "but j", a negative "only j"), the
    # first and the last position alleles that no other position takes, the middle ones further alleles in turn for as
    # long as there are any (two thirds of the gene at most, so that somebody is left).  The other mate keeps everybody
    # but one allele, so L & R shows the list's own mate.
    first, last, other = 0, n_allele - 1, 1
    pool = [int(j) for j in rng.permutation(np.arange(2, n_allele - 1))][:max(1, (2 * n_allele) // 3 - 3)]

    def takes(n):
        if n == 0:
            return []
        mid = [pool[q % len(pool)] for q in range(max(n - 2, 0))]
        return ([first] + mid + [last])[:n] if n > 1 else [last]

    for which in range(4):
        for n in lengths(g.G):
            js = takes(n)
            kind = "but" if which < 2 else "only"
            lst = [at[(kind, j)] for j in js]
            four = [[], [], [], []]
            four[which] = lst
            if which >= 2:
                four[which - 2] = [A]                   # the mate whose negatives these are names everybody first
            mate_other = 1 - (which & 1)
            four[mate_other] = [at[("but", other)]]
            fam(f"list {which} of {n}", *four)
    # ... and all four lists long at once, of different lengths, ids of no effect among them
    G4 = 4 * g.G
    fam("four long lists", [at[("but", j)] for j in takes(G4 + 1)], [at[("but", j)] for j in takes(2 * G4 - 1)][::-1],
        [at[("only", j)] for j in pool[:G4]] + [int(g.novel[0])], [at[("only", j)] for j in pool[1:2 * G4 + 2]])

    # ---- mates without positives, empty mates
    fam("negatives only, left", [], [A], [at[("only", 3)]], [])
    fam("negatives only, right", [at[("but", 2)]], [], [], [at[("only", 3)], A])
    fam("no positives at all", [], [], [at[("only", 3)]], [A])
    fam("nothing at all")
    fam("left empty, right not", [], [at[("but", 5)], at[("but", 6)]], [], [at[("only", 0)]])
    fam("right empty, left not", [at[("but", 5)]], [], [at[("only", n_allele - 1)]], [])

    # ---- ids that are not the gene's: positive -> the mate is empty; negative -> nothing
    for name, v, foreign in (("novel", g.novel[0], False), ("last novel", g.novel[-1], False),
                             ("below", g.below[-1], True), ("first below", g.below[0], True),
                             ("above", g.above[0], True), ("last above", g.above[-1], True)):
        fam(f"positive {name} id, left", [A, v], [at[("but", 1)]], [], [], foreign)
        fam(f"positive {name} id, right, first of its list", [at[("but", 1)]], [v, A], [], [], foreign)
        fam(f"positive {name} id alone", [v], [], [], [], foreign)
        fam(f"negative {name} id", [A], [at[("but", 1)]], [v], [v, at[("only", 2)]], foreign)
    # a list of 4 G ids of other genes and novel ones, positive and negative
    far = [int(v) for v in np.concatenate([g.below[:G4 // 2], g.novel[:G4 // 2]])]
    fam("a chunk of foreign positives", far, [at[("but", 1)]], [], [], True)
    fam("a chunk of foreign negatives", [A], [at[("but", 1)]], far, far[::-1], True)

    # ---- the gene's first and last variant
    fam("vbeg and vend - 1 positive", [g.vbeg], [g.vend - 1])
    fam("vend - 1 negative", [g.vbeg], [g.vbeg], [g.vend - 1], [])
    fam("vend - 1 positive, vbeg negative", [g.vend - 1], [g.vend - 1], [], [g.vbeg])

    # ---- named by both mates in exactly one word / in none
    for w in g.pair_words:
        fam(f"L & R in word {w} only", [at[("pairL", w)]], [at[("pairR", w)]])
        fam(f"L & R in word {w} only, mates swapped", [at[("pairR", w)]], [at[("pairL", w)]])
    fam("L & R empty: the union, first and last allele", [at[("only", 0)]], [at[("only", n_allele - 1)]])
    fam("each mate's negatives name the other mate's allele", [at[("only", 0)]], [at[("only", n_allele - 1)]],
        [at[("only", n_allele - 1)]], [at[("only", 0)]])
    fam("each mate's negatives name its own allele", [at[("only", 0)], A], [at[("only", n_allele - 1)]],
        [at[("only", 0)]], [at[("only", 1)]])
    fam("L & R empty: the union of two wide sets", [A], [A], [at[("pairL", 0)]], [at[("but", 1)], NONE])
    for j in sorted({0, 31, 32, n_allele - 1} | {b + d for b in range(32, n_allele, 32) for d in (-1, 0)}):
        if j < n_allele:
            fam(f"only allele {j}", [at[("only", j)]], [A])
            fam(f"everybody but allele {j}", [A], [A], [at[("only", j)]], [])

    # ---- a positive id of every allele / of none
    fam("everybody twice", [A], [A])
    fam("nobody left, everybody right", [NONE], [A])
    fam("nobody twice", [NONE], [NONE])
    fam("nobody among positives", [A, NONE, A], [A])
    fam("nobody as a negative", [A], [A], [NONE], [NONE])

    # ---- random short lists over the random rows at the end, the filler in the middle and the favouring rows
    middle = g.filler[np.linspace(0, len(g.filler) - 1, 24).astype(np.int64)] if len(g.filler) else g.rnd[:24]
    where = np.concatenate([g.rnd, middle, [at[("fav", k)] for k in range(8)]])
    for k in range(40):
        n = rng.integers(0, 4, 4)
        four = [rng.choice(where, int(m)).tolist() for m in n]
        if k % 5 == 4:
            four[2].append(int(g.novel[k % len(g.novel)]))
        fam(f"random {k}", *four)
    fam("the last variant and a middle one", [g.rnd[-1]], [middle[len(middle) // 2]])
    fam("middle rows", [middle[0]], [A], [middle[-1]], [middle[1]])
    return fams


def favouringRows(g: Gene, n: int) -> list[list[list[int]]]:
    """``n`` pairs that name one ``fav`` row each: their sets favour alleles 3 and 7."""
    return [[[g.at[("fav", k % g.N_FAV)]], [], [], []] for k in range(n)]
