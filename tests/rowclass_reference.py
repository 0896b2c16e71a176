"""numpy statement of the row classes of csrc/gk_rowclass.hip (helper of the row-class tests, not a test) and the hand-built
genes those tests share.

The KEPT sequence of a row is what the compatibility kernel multiplies over: the row's ids in CSR order (lpv, rpv, lnv,
rnv), each with its sign (negative = from lnv / rnv), without the ids whose drop flag has the bit of that sign (bit 0:
dropped from positive lists, bit 1: from negative ones).  Ids outside the gene's span stay: they are factors.  Where
the left mate's sub-list ends and the right mate's begins is not part of it; where the positives end is (the sign)."""
from __future__ import annotations

import numpy as np

import compat_reference as cr


def keptSequence(off, ids, row: int, vflag) -> tuple:
    """((id, sign), ...) of one CSR row: sign 0 = positive, 1 = negative."""
    b, mid, e = int(off[4 * row]), int(off[4 * row + 2]), int(off[4 * row + 4])
    return tuple((int(ids[k]), int(k >= mid)) for k in range(b, e) if not int(vflag[ids[k]]) & (1 if k < mid else 2))


def classOf(off, ids, rows, vflag) -> np.ndarray:
    """Class of every listed row: classes numbered by their lowest row, in row order."""
    first: dict[tuple, int] = {}
    out = np.empty(len(rows), dtype=np.uint32)
    for i, r in enumerate(rows):
        out[i] = first.setdefault(keptSequence(off, ids, int(r), vflag), len(first))
    return out


# ------------------------------------------------------------------------------------------------- the hand-built gene
# variants [0, 10) and [310, 340) belong to other genes, [340, 360) are novel; of the gene's own [10, 310):
#   [200, 280) are dropped from both sides (80 ids: more than a chunk of 64), 100 .. 104 from the positive lists only,
#   105 .. 109 from the negative lists only
VBEG, VEND, N_TOTAL = 10, 310, 360
DROPPED = list(range(200, 280))
KEEPABLE = [v for v in range(VBEG, 200) if not 100 <= v < 110]


def geneFlags() -> np.ndarray:
    vflag = np.zeros(N_TOTAL, dtype=np.uint8)
    vflag[DROPPED] = 3
    vflag[100:105] = 1
    vflag[105:110] = 2
    vflag[[3, 320, 345]] = 3          # ids outside the gene and a novel one carry flags too
    return vflag


def geneBits(n_allele: int, seed: int = 5) -> np.ndarray:
    """Even variants are carried by nine alleles in ten, odd ones by one in ten: a row of a dozen ids mismatches some
    alleles once or twice and others nearly everywhere."""
    rng = np.random.default_rng(seed + n_allele)
    p = np.where(np.arange(VEND - VBEG) % 2 == 0, 0.9, 0.1)[:, None]
    return rng.random((VEND - VBEG, n_allele)) < p


def distinctRow(i: int) -> list:
    """A row whose kept sequence names ``i`` (< 4096): bit b of i decides whether variant 10 + 2 b is seen or not."""
    pos = [VBEG + 2 * b for b in range(12) if i >> b & 1]
    neg = [VBEG + 2 * b for b in range(12) if not i >> b & 1]
    return [pos[:len(pos) // 2], pos[len(pos) // 2:], neg[:1], neg[1:]]


TEMPLATES = [
    [[12, 14, 16], [40, 42], [13, 15], [41]],
    [[12, 14], [16, 40, 42, 44], [], [13, 15, 41]],
    [[20], [], [21, 23, 25, 27, 29, 31], []],
]


def patternLists(pattern: str, n: int) -> tuple[list, int]:
    """(the rows' lists, the number of classes) of ``n`` rows laid out as ``pattern``."""
    if pattern == "distinct":
        return [distinctRow(i) for i in range(n)], n
    if pattern == "identical":
        return [TEMPLATES[0] for _ in range(n)], 1
    if pattern in ("two", "three"):
        k = 2 if pattern == "two" else 3
        return [TEMPLATES[i % k] for i in range(n)], min(k, n)
    if pattern == "tile edge":
        # rows 0 .. 14 distinct, row 15 -- the last of the first tile -- is the lowest row of a class whose other members
        # lie in the tiles behind it (every second row); the rows between are distinct
        lists = [TEMPLATES[2] if i == 15 or (i > 15 and i % 2) else distinctRow(i + 1) for i in range(n)]
        return lists, len({repr(x) for x in lists})
    raise ValueError(pattern)


def packed(lists, filler_every: int = 0):
    """(off, ids, rows) of ``lists``; with ``filler_every`` an unlisted CSR row lies in front of every such listed row."""
    csr, rows = [], []
    for i, row in enumerate(lists):
        if filler_every and i % filler_every == 0:
            csr.append([[11, 33], [], [55], []])
        rows.append(len(csr))
        csr.append(row)
    off, ids = cr.packLists(csr)
    return off, ids, np.array(rows, dtype=np.int32)
