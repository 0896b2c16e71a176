"""
Copy dosage of each called allele (``--call-dosage``).  An extension: the reference has no counterpart.

The likelihood search cannot see copies: a set's value is ``sum_r max_{a in S} log_probs[r, a]``
(typing_mulit_allele.py:540-542, 569), so ``(A, A, B)``, ``(A, B, B)`` and ``(A, B)`` score the same and the doubled allele is
chosen on ``fraction`` alone.  This module asks the reads how many copies of each called allele they support, under the
mixture model "a read comes from called allele k with share theta_k":

``l(theta) = sum_r log10 sum_k theta_k p[r, k] = const + sum_r log10 sum_k theta_k 999^-(b_k - m1)``

with ``b_k = miss8[k][r]`` the row's bytes of the ``u8`` mismatch table the search left in HBM (``DeviceModel.missFor``;
``p = .999^(n - m) .001^m``) and ``m1`` their minimum.

1. the called set and its columns of the table (``call_report.calledSet``);
2. ``gk_call_patterns`` (``calldosage_patterns``, csrc/gk_calldosage.hip) collapses the rows over the called columns into
   (pattern ``d = b - m1``, count) pairs in exact integers; the patterns are sorted, so every float sum below has one order;
3. ``solveDosage``: plain EM on the patterns from the called shares ``copies / cn`` -- monotone, and it stays on the simplex --
   then the integer compositions at ``cn - 1``, ``cn`` and ``cn + 1`` around the free optimum.  No search runs again.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .utils import logger

FIRST_SLOTS = 4096               # patterns the first call can hold
MAX_SLOTS = 1 << 21              # ... and the last: 8 times as many per retry
ITER_MAX = 5000
TOLERANCE = 1e-10                # on kkt = max_k theta_k |g_k - 1|
ABSENT = 255                     # a pattern byte: the allele cannot have produced the read

CALL_DOSAGE_COLUMNS = ["gene", "cn", "reads", "out_of_range", "patterns", "iterations", "converged", "kkt", "loglik_called",
                       "loglik_free", "allele", "copies", "share", "dosage", "tied_with", "minus_set", "minus_delta",
                       "same_set", "same_delta", "plus_set", "plus_delta", "scope"]


@dataclass
class Solution:
    """``solveDosage``'s answer.  ``theta``: the shares at the end of the EM; ``kkt = max_k theta_k |g_k - 1|`` there;
    ``compositions``: total copies -> (copies per column, delta = l(copies / total) - loglik_called) for ``cn - 1``, ``cn``
    and ``cn + 1`` (no entry for a total of 0)."""

    theta: np.ndarray
    iterations: int
    converged: bool
    kkt: float
    loglik_called: float
    loglik_free: float
    compositions: dict[int, tuple[tuple[int, ...], float]] = field(default_factory=dict)


@dataclass
class DosageAllele:
    """One distinct allele of the called set.  ``share`` = theta_k, ``dosage`` = theta_k cn (None for a gene without a
    read in range); ``tied_with``: the other called alleles whose columns equal this one's on every read -- the reads
    cannot tell them apart, only the SUM of their shares is estimated and the EM keeps their starting ratio."""

    allele: str
    copies: int
    share: float | None
    dosage: float | None
    tied_with: list[str] = field(default_factory=list)


@dataclass
class CallDosage:
    """Dosage of one gene's called set.  ``reads``: rows of the table; ``out_of_range``: those whose every called byte is
    255 (``gk_call_fit``'s bin 17; they carry no pattern); ``patterns`` [n, K] (sorted) with ``counts`` [n].
    ``minus`` / ``same`` / ``plus``: ([(allele, copies), ...], delta) of the best integer composition at ``cn - 1`` / ``cn`` /
    ``cn + 1`` copies, ``delta`` = its log10 likelihood minus that of the called composition (the units of ``value``); None
    where there is none.  ``scope`` as ``CallFit.extra_scope``."""

    cn: int
    reads: int
    out_of_range: int
    patterns: np.ndarray
    counts: np.ndarray
    iterations: int | None
    converged: bool | None
    kkt: float | None
    loglik_called: float | None
    loglik_free: float | None
    alleles: list[DosageAllele] = field(default_factory=list)
    minus: tuple[list[tuple[str, int]], float] | None = None
    same: tuple[list[tuple[str, int]], float] | None = None
    plus: tuple[list[tuple[str, int]], float] | None = None
    scope: str = "all"


# ------------------------------------------------------------------------------------------------ the device
def callPatterns(dev, miss8, ldm: int, n_rows: int, n_table_cols: int, cols: np.ndarray, n_slots: int):
    """``gk_call_patterns`` with ``n_slots`` slots: (patterns uint8 [n, 16], counts int64 [n], out_of_range, unplaced)."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    patterns = np.zeros((n_slots, 16), dtype=np.uint8)
    counts = np.zeros(n_slots, dtype=np.uint64)
    n = np.zeros(1, dtype=np.int64)
    out_of_range, unplaced = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    check(lib().gk_call_patterns(dev.ctx, miss8.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, len(cols), n_slots,
                                 patterns.ctypes.data, counts.ctypes.data, n.ctypes.data, out_of_range.ctypes.data,
                                 unplaced.ctypes.data))
    found = int(n[0])
    return patterns[:found].copy(), counts[:found].astype(np.int64), int(out_of_range[0]), int(unplaced[0])


def sortedPatterns(patterns: np.ndarray, counts: np.ndarray, k: int):
    """The first ``k`` bytes of the patterns in lexicographic order, with their counts."""
    patterns = np.asarray(patterns, dtype=np.uint8).reshape(-1, patterns.shape[1] if patterns.ndim == 2 else 16)[:, :k]
    order = np.lexsort(patterns.T[::-1]) if len(patterns) else np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(patterns[order]), np.asarray(counts, dtype=np.int64)[order]


def patternsOfColumns(dev, miss8, ldm: int, n_rows: int, n_table_cols: int, cols: np.ndarray,
                      first_slots: int = FIRST_SLOTS, max_slots: int = MAX_SLOTS):
    """The complete sorted pattern list of the listed columns: (patterns [n, K], counts [n], out_of_range), the slots
    grown 8-fold while rows stay unplaced; None when ``max_slots`` do not hold the patterns."""
    n_slots = int(first_slots)
    while True:
        patterns, counts, out_of_range, unplaced = callPatterns(dev, miss8, ldm, n_rows, n_table_cols, cols, n_slots)
        if unplaced == 0:
            assert int(counts.sum()) + out_of_range == n_rows
            return (*sortedPatterns(patterns, counts, len(cols)), out_of_range)
        if n_slots >= max_slots:
            return None
        n_slots = min(n_slots * 8, int(max_slots))


# ------------------------------------------------------------------------------------------------ the solver
def patternWeights(patterns: np.ndarray) -> np.ndarray:
    """``w[c, k] = 999 ** -d``, 0 where ``d == 255``."""
    d = np.asarray(patterns, dtype=np.float64)
    return np.where(np.asarray(patterns) == ABSENT, 0.0, 999.0 ** -d)


def mixture(w: np.ndarray, theta: np.ndarray) -> np.ndarray:
    """``s_c = sum_j theta_j w[c, j]``, the columns added in ascending order."""
    s = np.zeros(w.shape[0], dtype=np.float64)
    for j in range(w.shape[1]):
        s = s + theta[j] * w[:, j]
    return s


def logLikelihood(w: np.ndarray, counts: np.ndarray, theta: np.ndarray) -> float:
    """``l(theta) = sum_c n_c log10 s_c``; -inf when a pattern with rows has no share at all."""
    with np.errstate(divide="ignore"):
        return float(np.sum(counts * np.log10(mixture(w, theta))))


def largestRemainder(x: np.ndarray, total: int) -> tuple[int, ...]:
    """``x`` (sum ``total``) rounded to integers of the same sum: floors, then one more to the largest remainders, the
    lower column first among equal ones."""
    x = np.asarray(x, dtype=np.float64)
    low = np.floor(x).astype(np.int64)
    order = np.argsort(-(x - low), kind="stable")
    out = low.copy()
    for j in order[:max(0, int(total) - int(low.sum()))]:
        out[j] += 1
    return tuple(int(c) for c in out)


def compositionCandidates(start: tuple[int, ...], called: tuple[int, ...] | None) -> list[tuple[int, tuple[int, ...]]]:
    """(moves from ``start``, composition): ``start``, every move of one copy from a column that has one to another, and
    ``called`` when given; each composition once, with its fewest moves."""
    found = {start: 0}
    for i in range(len(start)):
        for j in range(len(start)):
            if i != j and start[i] >= 1:
                c = list(start)
                c[i] -= 1
                c[j] += 1
                found.setdefault(tuple(c), 1)
    if called is not None:
        found.setdefault(tuple(called), sum(abs(a - b) for a, b in zip(called, start)) // 2)
    return [(moves, c) for c, moves in found.items()]


def bestComposition(w, counts, theta, total: int, called: tuple[int, ...] | None):
    """The best integer composition of ``total`` copies near ``theta``: (copies, l(copies / total)).  Ties: fewer moves
    from the rounding of ``theta total``, then the lexicographically smaller composition."""
    start = largestRemainder(np.asarray(theta) * total, total)
    scored = [(-logLikelihood(w, counts, np.asarray(c, dtype=np.float64) / total), moves, c)
              for moves, c in compositionCandidates(start, called)]
    neg, _, c = min(scored)
    return c, -neg


def solveDosage(patterns: np.ndarray, counts: np.ndarray, copies, iter_max: int = ITER_MAX,
                tolerance: float = TOLERANCE) -> Solution:
    """EM for the shares of the K called alleles on (pattern, count) pairs, from ``copies / cn``: ``s = w theta``,
    ``g_k = sum_c n_c w[c, k] / s_c / N``, ``theta <- theta g``, until ``max_k theta_k |g_k - 1| <= tolerance`` or
    ``iter_max`` passes; then the integer compositions.  Needs at least one pattern."""
    copies = tuple(int(c) for c in copies)
    cn, k = sum(copies), len(copies)
    w = patternWeights(np.asarray(patterns)[:, :k])
    n = np.asarray(counts, dtype=np.float64)
    total = float(np.asarray(counts, dtype=np.int64).sum())
    called = np.asarray(copies, dtype=np.float64) / cn
    theta, iterations = called.copy(), 0
    if k == 1:
        converged, kkt = True, 0.0
    else:
        while True:
            s = mixture(w, theta)
            g = np.array([np.sum(n * w[:, j] / s) for j in range(k)]) / total
            kkt = float(np.max(theta * np.abs(g - 1.0)))
            converged = kkt <= tolerance
            if converged or iterations >= iter_max:
                break
            theta = theta * g
            iterations += 1
    loglik_called = logLikelihood(w, n, called)
    loglik_free = logLikelihood(w, n, theta)
    if loglik_free < loglik_called:      # rounding at a start that is the optimum already: the better point is reported
        theta, loglik_free = called.copy(), loglik_called
    out = Solution(theta=theta, iterations=iterations, converged=bool(converged), kkt=kkt, loglik_called=loglik_called,
                   loglik_free=loglik_free)
    for total_copies in (cn - 1, cn, cn + 1):
        if total_copies >= 1:
            c, value = bestComposition(w, n, theta, total_copies, copies if total_copies == cn else None)
            out.compositions[total_copies] = (c, value - loglik_called)
    return out


def tiedColumns(patterns: np.ndarray, k: int) -> list[list[int]]:
    """Per column the other columns that equal it on every pattern."""
    p = np.asarray(patterns)[:, :k]
    return [[j for j in range(k) if j != i and np.array_equal(p[:, i], p[:, j])] for i in range(k)]


# ------------------------------------------------------------------------------------------------ the report
def dosageOfCall(result, names=None) -> CallDosage | None:
    """The dosage of one gene's adopted result (the last step's ``TypingResult``).  ``names`` is accepted as ``fitCall``
    accepts it (the called names come from the result itself).  None -- with a warning -- when the result's sets do not sit
    on one device table, the model has no mismatch table, the called set has more than 16 distinct alleles, or the rows take
    more than 2^21 patterns."""
    called = calledSet(result, "call dosage", names)
    if called is None:
        return None
    n, k, cn, copies = called.reads, len(called.ids), called.cn, called.copies
    found = patternsOfColumns(called.model.dev, called.miss8, called.ldm, n, called.n_table_cols, called.cols)
    if found is None:
        logger.warning(f"[Allele] call dosage: the reads take more than {MAX_SLOTS} patterns over the called alleles; skipped")
        return None
    patterns, counts, out_of_range = found
    labels, scope = called.labels, called.scope
    if len(counts) == 0:      # every read out of range: nothing to estimate
        alleles = [DosageAllele(labels[j], copies[j], None, None) for j in range(k)]
        return CallDosage(cn=cn, reads=n, out_of_range=out_of_range, patterns=patterns, counts=counts, iterations=None,
                          converged=None, kkt=None, loglik_called=None, loglik_free=None, alleles=alleles, scope=scope)
    sol = solveDosage(patterns, counts, copies)
    tied = tiedColumns(patterns, k)
    alleles = [DosageAllele(labels[j], copies[j], float(sol.theta[j]), float(sol.theta[j]) * cn,
                            [labels[i] for i in tied[j]]) for j in range(k)]

    def named(total):
        if total not in sol.compositions:
            return None
        c, delta = sol.compositions[total]
        return [(labels[j], int(c[j])) for j in range(k)], float(delta)

    return CallDosage(cn=cn, reads=n, out_of_range=out_of_range, patterns=patterns, counts=counts, iterations=sol.iterations,
                      converged=sol.converged, kkt=sol.kkt, loglik_called=sol.loglik_called, loglik_free=sol.loglik_free,
                      alleles=alleles, minus=named(cn - 1), same=named(cn), plus=named(cn + 1), scope=scope)


def _cell(x) -> str:
    if x is None:
        return ""
    if isinstance(x, (bool, np.bool_)):
        return "1" if x else "0"
    if isinstance(x, (float, np.floating)):
        return repr(float(x))
    return str(x)


def _setCells(entry) -> list[str]:
    if entry is None:
        return ["", ""]
    pairs, delta = entry
    return [",".join(f"{a}:{c}" for a, c in pairs), repr(float(delta))]


def callDosageText(dosages: dict[str, CallDosage]) -> str:
    """``{result}.dosage.tsv``: tab separated, one row per gene and distinct called allele, the gene's own cells repeated
    on each of its rows; floats as their shortest exact text, ``converged`` as 0 / 1, sets as ``name:copies,...`` (copies
    of 0 included), ``tied_with`` comma separated, an empty cell where a value is undefined."""
    lines = ["\t".join(CALL_DOSAGE_COLUMNS)]
    for gene, d in dosages.items():
        head = [gene, d.cn, d.reads, d.out_of_range, len(d.counts), d.iterations, d.converged, d.kkt, d.loglik_called,
                d.loglik_free]
        tail = _setCells(d.minus) + _setCells(d.same) + _setCells(d.plus) + [d.scope]
        for a in d.alleles:
            cells = [_cell(x) for x in head + [a.allele, a.copies, a.share, a.dosage, ",".join(a.tied_with)]] + tail
            lines.append("\t".join(cells))
    return "\n".join(lines) + "\n"


# at the end, not at the top: call_report's table of reports names this module, and whichever of the two is imported first
# finds what it needs of the other already defined
from .call_report import calledSet  # noqa: E402
