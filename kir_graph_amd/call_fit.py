"""
Fit report of a likelihood call (``--call-fit``).

``.possible.tsv`` and ``--call-bootstrap`` compare the called set with other sets.  This module says how well the called
set explains the reads in absolute terms, and what each called copy contributes -- in exact integers, from the ``u8``
mismatch table ``miss8[column][read]`` the search left in HBM (``DeviceModel.missFor``).  The search's value of a set S is
``c N - (3 + c) M(S)`` with ``c = log10(.999)``, ``N`` the reads' listed variants and ``M(S) = sum_r min_{a in S} miss[r, a]``
(csrc/gk_bound.hip; typing_mulit_allele.py:540-542, 569): one mismatching observation is worth about 2.9996 of ``value``.

1. the called set and its columns of the table (``call_report.calledSet``);
2. ``gk_call_fit`` (``callfit_profile``): the histogram of the reads' smallest mismatch count ``m1`` over the called
   columns, ``M = sum m1``, per called allele the reads it explains best (ties included), the reads it alone explains best
   and how much ``M`` grows without it; ``d_min[r] = m1``;
3. ``gk_call_fit_extra`` (``callfit_extra``): ``with[a] = sum_r min(d_min[r], miss8[a][r])`` for every column of the table;
   ``gain = M - with[a]`` is what allele ``a`` as one more copy would explain.  No search runs again.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .utils import logger

MAX_EXTRA = 64                   # extra alleles listed per gene
N_BINS = 18                      # m1 == 0 .. 15, 16 .. 254, 255 (out of range)

CALL_FIT_COLUMNS = ["gene", "cn", "reads", "explained", "miss1", "miss2", "miss3plus", "out_of_range", "mismatches",
                    "allele", "copies", "best", "unique", "only_explains", "extra_scope"]


@dataclass
class CalledAllele:
    """One distinct allele of the called set: the reads on which it is (among) the best of the set, those on which it
    alone is, and ``only_explains`` = M of the set without it minus M (None for a set of one distinct allele)."""

    allele: str
    copies: int
    best: int
    unique: int
    only_explains: int | None


@dataclass
class CallFit:
    """Fit of one gene's called set.  ``hist[i]``: reads whose smallest mismatch count over the called alleles is ``i``
    (``i < 16``), 16 .. 254 (bin 16), or the table's 255 = a count >= 100 or a product out of range (bin 17,
    ``out_of_range``); ``mismatches`` = M, the bytes summed as stored.  ``extra``: (allele, gain) of the non-called
    alleles that would explain the most as one more copy, ``gain = M - M(called + allele)`` > 0, largest first;
    ``extra_scope``: ``"all"`` when every allele of the gene was looked at, ``"candidates"`` when the table holds the
    exon-first candidates only."""

    cn: int
    reads: int
    hist: np.ndarray
    mismatches: int
    out_of_range: int
    alleles: list[CalledAllele] = field(default_factory=list)
    extra: list[tuple[str, int]] = field(default_factory=list)
    extra_scope: str = "all"


def profileColumns(dev, miss8, ldm: int, n_rows: int, n_table_cols: int, cols: np.ndarray, want_min: bool):
    """``gk_call_fit`` on the listed columns: (hist [18], per column [K, 3] = best / unique / only, M, d_min buffer or
    None).  The caller frees ``d_min``."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    hist = np.zeros(N_BINS, dtype=np.uint64)
    per_col = np.zeros((len(cols), 3), dtype=np.uint64)
    m = np.zeros(1, dtype=np.uint64)
    d_min = dev.alloc(n_rows, np.uint8) if want_min else None
    try:
        check(lib().gk_call_fit(dev.ctx, miss8.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, len(cols), hist.ctypes.data,
                                per_col.ctypes.data, m.ctypes.data, d_min.ptr if d_min is not None else 0))
    except Exception:
        if d_min is not None:
            d_min.free()
        raise
    return hist.astype(np.int64), per_col.astype(np.int64), int(m[0]), d_min


def extraSums(dev, miss8, ldm: int, n_rows: int, n_table_cols: int, d_min) -> np.ndarray:
    """``gk_call_fit_extra``: ``sum_r min(d_min[r], miss8[a][r])`` of every column of the table."""
    out = np.zeros(n_table_cols, dtype=np.uint64)
    check(lib().gk_call_fit_extra(dev.ctx, miss8.ptr, ldm, n_rows, n_table_cols, d_min.ptr, out.ctypes.data))
    return out.astype(np.int64)


def largestGains(gain: np.ndarray, called: np.ndarray, extra: int) -> list[tuple[int, int]]:
    """(column, gain) of the ``extra`` largest gains over the non-called columns, the lower column first among equal
    gains, gains of 0 dropped."""
    gain = np.asarray(gain, dtype=np.int64).copy()
    gain[np.asarray(called, dtype=np.int64)] = 0
    order = np.argsort(-gain, kind="stable")[:max(0, int(extra))]
    return [(int(a), int(gain[a])) for a in order if gain[a] > 0]


def fitCall(result, extra: int = 3, names=None) -> CallFit | None:
    """The fit of one gene's adopted result (the last step's ``TypingResult``).  ``extra``: how many non-called alleles
    to list (0: the second kernel and ``d_min`` are skipped).  ``names``: allele ordinal -> name for a result that does
    not carry the map itself (the merged result of exon-first).  None -- with a warning -- when the result's sets do not
    sit on one device table, the model has no mismatch table, or the called set has more than 16 distinct alleles."""
    if not 0 <= int(extra) <= MAX_EXTRA:
        raise ValueError(f"call fit: extra must lie in 0 .. {MAX_EXTRA}, got {extra}")
    called = calledSet(result, "call fit", names)
    if called is None:
        return None
    dev, n, extra = called.model.dev, called.reads, int(extra)
    table = (called.miss8, called.ldm, n, called.n_table_cols)
    hist, per_col, m, d_min = profileColumns(dev, *table, called.cols, want_min=extra > 0)
    listed: list[tuple[str, int]] = []
    try:
        if extra > 0:
            with_a = extraSums(dev, *table, d_min)
            for col, gain in largestGains(m - with_a, called.cols, extra):
                if called.names is None:
                    logger.warning("[Allele] call fit: no allele names for the table's columns; extra alleles not listed")
                    break
                listed.append((called.nameOf(col), gain))
    finally:
        if d_min is not None:
            d_min.free()
    k = len(called.ids)
    alleles = [CalledAllele(allele=called.labels[j], copies=called.copies[j], best=int(per_col[j, 0]),
                            unique=int(per_col[j, 1]), only_explains=int(per_col[j, 2]) if k > 1 else None)
               for j in range(k)]
    return CallFit(cn=called.cn, reads=n, hist=hist, mismatches=m, out_of_range=int(hist[17]), alleles=alleles,
                   extra=listed, extra_scope=called.scope)


def callFitText(fits: dict[str, CallFit]) -> str:
    """``{result}.fit.tsv``: tab separated, one row per gene and distinct called allele, the gene's own cells repeated on
    each of its rows, then ``extra_i`` / ``gain_i`` up to the longest list of extras; integers as integers, an empty
    cell where a value is undefined.  ``explained`` = reads without a mismatch, ``miss3plus`` = bins 3 .. 16."""
    width = max((len(f.extra) for f in fits.values()), default=0)
    header = CALL_FIT_COLUMNS + [c for i in range(width) for c in (f"extra_{i + 1}", f"gain_{i + 1}")]
    lines = ["\t".join(header)]
    for gene, f in fits.items():
        h = [int(x) for x in f.hist]
        head = [gene, f.cn, f.reads, h[0], h[1], h[2], sum(h[3:17]), f.out_of_range, f.mismatches]
        tail = [f.extra_scope] + [x for pair in f.extra for x in pair] + [""] * (2 * (width - len(f.extra)))
        for a in f.alleles:
            cells = head + [a.allele, a.copies, a.best, a.unique, "" if a.only_explains is None else a.only_explains] + tail
            lines.append("\t".join(str(c) for c in cells))
    return "\n".join(lines) + "\n"


# at the end, not at the top: call_report's table of reports names this module, and whichever of the two is imported first
# finds what it needs of the other already defined
from .call_report import calledSet  # noqa: E402
