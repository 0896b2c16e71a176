"""
Alternatives of each called allele of a likelihood call (``--call-alternatives``).

The likelihood strategies pick one allele set per gene among candidates that tie all the time.  This
module says, for every called allele, which other alleles could stand in for it and down to which field of its name the
reads resolve the call -- in exact integers, from the ``u8`` mismatch table ``miss8[column][read]`` the search left in HBM
(``DeviceModel.missFor``).  With ``M(S) = sum_r min_{a in S} miss[r, a]`` the search's value of a set is
``c N - (3 + c) M(S)`` (call_fit.py): one unit of ``delta`` below is about 2.9996 of ``value``.

1. the called set and its columns of the table (``call_report.calledSet``);
2. ``gk_call_swap`` (``callswap_rows``, ``callswap_sums``): for every called allele ``k`` and every column ``a`` of the
   table the swap ``S(k -> a)`` that replaces every copy of ``k`` by ``a``: ``loss[k][a]`` / ``rows_for[k][a]`` = the
   mismatches added on, and the number of, the reads that prefer ``k``; ``gain[a]`` / ``rows_against[a]`` = the mismatches
   removed on, and the number of, the reads that prefer ``a``; ``delta = loss - gain = M(S(k -> a)) - M(S)``;
3. every column ``a != k`` gets a class: ``better`` (delta < 0), ``identical`` (loss == 0 and gain == 0: no read tells the
   two apart given the rest of the call), ``balanced`` (delta == 0, loss > 0), ``near`` (0 < delta <= within).  No search
   runs again.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .utils import logger

MAX_WITHIN = 64                  # the largest delta still listed as near
MAX_LISTED = 256                 # alternatives listed per called allele
CLASSES = ("better", "identical", "balanced", "near")

CALL_ALTERNATIVES_COLUMNS = ["gene", "cn", "reads", "mismatches", "out_of_range", "scope", "allele", "copies", "resolved",
                             "n_better", "n_identical", "n_balanced", "n_near", "alternative", "class", "delta", "loss", "gain",
                             "rows_for", "rows_against"]
CALL_ALTERNATIVES_HEADER = (
    "# scope candidates: the table holds the exon-first candidates of the gene only; the counts and `resolved` then speak "
    "about those candidates, not about every allele of the gene (scope all: every allele was looked at)\n"
    "# delta = loss - gain = mismatches of the call with `alternative` in the place of `allele`, minus `mismatches`; one unit "
    "is about 2.9996 of the search's value.  With out_of_range > 0 every delta is a bound: those reads carry the byte 255\n")


@dataclass
class Alternative:
    """Allele ``allele`` in the place of a called one: ``delta = loss - gain``; ``rows_for`` reads prefer the called
    allele (``loss`` mismatches more without it), ``rows_against`` prefer this one (``gain`` mismatches fewer with it)."""

    allele: str
    cls: str
    delta: int
    loss: int
    gain: int
    rows_for: int
    rows_against: int


@dataclass
class CalledAlternatives:
    """One distinct allele of the called set: the number of alleles of every class (always in full), the first
    ``max_listed`` of them, and ``resolved`` = the name cut to the field the reads resolve."""

    allele: str
    copies: int
    resolved: str
    n_better: int
    n_identical: int
    n_balanced: int
    n_near: int
    listed: list[Alternative] = field(default_factory=list)


@dataclass
class CallAlternatives:
    """Alternatives of one gene's called set.  ``mismatches`` = M, the bytes summed as stored; ``out_of_range``: reads whose
    smallest byte over the called alleles is the table's 255; ``scope``: ``"all"`` when every allele of the gene was looked
    at, ``"candidates"`` when the table holds the exon-first candidates only."""

    cn: int
    reads: int
    mismatches: int
    out_of_range: int
    scope: str = "all"
    alleles: list[CalledAlternatives] = field(default_factory=list)


def swapSums(dev, miss8, ldm: int, n_rows: int, n_table_cols: int, cols: np.ndarray):
    """``gk_call_swap`` on the listed columns: (loss [K, A], rows_for [K, A], gain [A], rows_against [A], M, out of range)."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    k = len(cols)
    loss = np.zeros((k, n_table_cols), dtype=np.uint64)
    rows_for = np.zeros((k, n_table_cols), dtype=np.uint64)
    gain = np.zeros(n_table_cols, dtype=np.uint64)
    against = np.zeros(n_table_cols, dtype=np.uint64)
    m, beyond = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    check(lib().gk_call_swap(dev.ctx, miss8.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, k, loss.ctypes.data,
                             rows_for.ctypes.data, gain.ctypes.data, against.ctypes.data, m.ctypes.data, beyond.ctypes.data, 0))
    return (loss.astype(np.int64), rows_for.astype(np.int64), gain.astype(np.int64), against.astype(np.int64), int(m[0]),
            int(beyond[0]))


def classOf(loss: int, gain: int, within: int) -> str | None:
    """The class of a swap, None for one that costs more than ``within``."""
    delta = loss - gain
    if delta < 0:
        return "better"
    if delta == 0:
        return "identical" if loss == 0 else "balanced"
    return "near" if delta <= within else None


def rankAlternatives(loss: np.ndarray, gain: np.ndarray, own: int, within: int, max_listed: int):
    """The swaps of one called column ``own`` against every other column: (count per class, the listed columns as
    (column, class)): ``better`` by delta, most negative first, then ``identical``, ``balanced``, ``near`` by delta; the
    lower column first among equals; at most ``max_listed``."""
    loss, gain = np.asarray(loss, dtype=np.int64), np.asarray(gain, dtype=np.int64)
    found = []
    counts = dict.fromkeys(CLASSES, 0)
    for a in range(len(gain)):
        cls = None if a == own else classOf(int(loss[a]), int(gain[a]), within)
        if cls is not None:
            counts[cls] += 1
            delta = int(loss[a] - gain[a])
            found.append((CLASSES.index(cls), delta if cls in ("better", "near") else 0, a, cls))
    found.sort()
    return counts, [(a, cls) for _, _, a, cls in found[:max(0, int(max_listed))]]


def nameFields(name: str) -> tuple[str, str] | None:
    """(``GENE*``, digits) of a name that is ``GENE*`` plus 3 to 7 digits, else None."""
    gene, star, digits = name.partition("*")
    if not star or not gene or not digits.isdigit() or not digits.isascii() or not 3 <= len(digits) <= 7:
        return None
    return gene + star, digits


def resolvedName(called: str, others: list[str]) -> str:
    """``called`` cut to the longest of its 7-, 5- or 3-digit fields (the digits after ``*``, split 3 + 2 + 2) that every
    name of ``others`` shares: the whole name when there are none, ``GENE*`` when not even three digits are shared.  A
    name that is not ``GENE*`` plus 3 to 7 digits is compared as a whole: it shares no field with a different name."""
    if not others:
        return called
    mine = nameFields(called)
    if mine is None:
        if all(o == called for o in others):
            return called
        return called.partition("*")[0] + "*" if "*" in called else ""
    gene, digits = mine
    theirs = [nameFields(o) for o in others]
    for width in (7, 5, 3):
        if width <= len(digits) and all(t is not None and t[0] == gene and t[1][:width] == digits[:width] and
                                        len(t[1]) >= width for t in theirs):
            return gene + digits[:width]
    return gene


def alternativesFromSums(loss, rows_for, gain, against, cols, called_names, copies, name_of, cn: int, reads: int, m: int,
                         out_of_range: int, scope: str, within: int, max_listed: int) -> CallAlternatives:
    """The report from the sums of ``gk_call_swap``: ``cols`` the called columns, ``called_names`` / ``copies`` theirs,
    ``name_of(column)`` the name of any column of the table."""
    out = CallAlternatives(cn=int(cn), reads=int(reads), mismatches=int(m), out_of_range=int(out_of_range), scope=scope)
    for k, col in enumerate(cols):
        counts, listed = rankAlternatives(loss[k], gain, int(col), within, max_listed)
        rows = [Alternative(allele=name_of(a), cls=cls, delta=int(loss[k][a] - gain[a]), loss=int(loss[k][a]), gain=int(gain[a]),
                            rows_for=int(rows_for[k][a]), rows_against=int(against[a])) for a, cls in listed]
        # `resolved` speaks about every alternative that costs nothing, listed or not
        free = [name_of(a) for a in range(len(gain))
                if a != int(col) and classOf(int(loss[k][a]), int(gain[a]), within) in ("better", "identical", "balanced")]
        out.alleles.append(CalledAlternatives(allele=called_names[k], copies=int(copies[k]),
                                              resolved=resolvedName(called_names[k], free), n_better=counts["better"],
                                              n_identical=counts["identical"], n_balanced=counts["balanced"],
                                              n_near=counts["near"], listed=rows))
    return out


def alternativesOfCall(result, within: int = 1, max_listed: int = 20, names=None) -> CallAlternatives | None:
    """The alternatives of one gene's adopted result (the last step's ``TypingResult``).  ``within``: the largest
    ``delta`` still listed as ``near``; ``max_listed``: alternatives listed per called allele.  ``names``: allele ordinal
    -> name for a result that does not carry the map itself (the merged result of exon-first).  None -- with a warning --
    when the result's sets do not sit on one device table, the model has no mismatch table, or the called set has more
    than 16 distinct alleles."""
    if not 0 <= int(within) <= MAX_WITHIN:
        raise ValueError(f"call alternatives: within must lie in 0 .. {MAX_WITHIN}, got {within}")
    if not 1 <= int(max_listed) <= MAX_LISTED:
        raise ValueError(f"call alternatives: max_listed must lie in 1 .. {MAX_LISTED}, got {max_listed}")
    called = calledSet(result, "call alternatives", names)
    if called is None:
        return None
    if called.names is None:
        logger.warning("[Allele] call alternatives: no allele names for the table's columns; skipped")
        return None
    cols = called.cols
    loss, rows_for, gain, against, m, beyond = swapSums(called.model.dev, called.miss8, called.ldm, called.reads,
                                                        called.n_table_cols, cols)
    return alternativesFromSums(loss, rows_for, gain, against, cols.tolist(), called.labels, called.copies, called.nameOf,
                                called.cn, called.reads, m, beyond, called.scope, int(within), int(max_listed))


def callAlternativesText(calls: dict[str, CallAlternatives]) -> str:
    """``{result}.alternatives.tsv``: two ``#`` lines (what ``scope`` and ``delta`` mean), then tab separated one row per
    gene, distinct called allele and listed alternative, the gene's and the called allele's own cells repeated on each of
    their rows; a called allele without an alternative gets one row with empty alternative cells.  Integers as integers."""
    lines = ["\t".join(CALL_ALTERNATIVES_COLUMNS)]
    for gene, c in calls.items():
        head = [gene, c.cn, c.reads, c.mismatches, c.out_of_range, c.scope]
        for a in c.alleles:
            mine = head + [a.allele, a.copies, a.resolved, a.n_better, a.n_identical, a.n_balanced, a.n_near]
            tails = [[x.allele, x.cls, x.delta, x.loss, x.gain, x.rows_for, x.rows_against] for x in a.listed] or [[""] * 7]
            lines += ["\t".join(str(v) for v in mine + t) for t in tails]
    return CALL_ALTERNATIVES_HEADER + "\n".join(lines) + "\n"


# at the end, not at the top: call_report's table of reports names this module, and whichever of the two is imported first
# finds what it needs of the other already defined
from .call_report import calledSet  # noqa: E402
