"""Brute-force restatement of the copy dosage of a call (kir_graph_amd/call_dosage.py, csrc/gk_calldosage.hip): the patterns by
np.unique over the rows of the expanded table, the EM and the log10 likelihood as plain Python loops with math.fsum, and
again in np.longdouble.  Nothing here shares code with the package."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

LD = np.longdouble
BOUND_CEILING = 1e-9      # no case's bound may exceed this


def patterns(table: np.ndarray, cols) -> tuple[np.ndarray, np.ndarray, int]:
    """``table`` uint8 [columns][rows]: (distinct patterns [n, K] in lexicographic order, their row counts, rows whose
    every called byte is 255)."""
    b = np.asarray(table)[np.asarray(cols, dtype=np.int64)].T.astype(np.int64)      # [rows, K]
    m1 = b.min(axis=1)
    out_of_range = int((m1 == 255).sum())
    b = b[m1 < 255]
    d = np.where(b == 255, 255, b - b.min(axis=1, keepdims=True)).astype(np.uint8)
    if len(d) == 0:
        return np.zeros((0, len(cols)), dtype=np.uint8), np.zeros(0, dtype=np.int64), out_of_range
    uniq, counts = np.unique(d, axis=0, return_counts=True)
    return uniq, counts.astype(np.int64), out_of_range


class Run(NamedTuple):
    theta: list
    iterations: int
    converged: bool
    kkt: float
    loglik_called: float
    loglik_free: float


def _weights(pats, real):
    return [[real(0) if int(d) == 255 else real(999) ** -int(d) for d in row] for row in pats]


def _loglik(w, counts, theta, real, total):
    log10 = math.log10 if real is float else np.log10
    terms = []
    for row, n in zip(w, counts):
        s = total(t * x for t, x in zip(theta, row))
        terms.append(real(int(n)) * log10(s) if s > 0 else real(-math.inf))
    return total(terms)


def em(pats, counts, copies, passes: int | None = None, iter_max: int = 5000, tolerance: float = 1e-10, dtype=float) -> Run:
    """Plain EM from ``copies / cn``.  ``dtype=float``: Python floats, every sum by math.fsum; ``dtype=np.longdouble``: the
    same in extended precision with sequential sums.  ``passes``: exactly that many updates, no stop test."""
    real = float if dtype is float else LD
    total = math.fsum if dtype is float else (lambda it: sum(it, LD(0)))
    k, cn = len(copies), sum(int(c) for c in copies)
    w = _weights(np.asarray(pats)[:, :k], real)
    n_all = real(int(np.sum(counts)))
    called = [real(int(c)) / real(cn) for c in copies]
    theta, done, converged, kkt = list(called), 0, False, real(0)
    if k == 1:
        converged = True
    else:
        while True:
            s = [total(t * x for t, x in zip(theta, row)) for row in w]
            g = [total(real(int(n)) * row[j] / sc for row, n, sc in zip(w, counts, s)) / n_all for j in range(k)]
            kkt = max(t * abs(x - real(1)) for t, x in zip(theta, g))
            converged = bool(kkt <= tolerance)
            if passes is None and (converged or done >= iter_max):
                break
            if passes is not None and done >= passes:
                break
            theta = [t * x for t, x in zip(theta, g)]
            done += 1
    return Run(theta, done, converged, float(kkt), _loglik(w, counts, called, real, total),
               _loglik(w, counts, theta, real, total))


def loglik(pats, counts, theta, dtype=float):
    real = float if dtype is float else LD
    total = math.fsum if dtype is float else (lambda it: sum(it, LD(0)))
    w = _weights(np.asarray(pats)[:, :len(theta)], real)
    return _loglik(w, counts, [real(t) for t in theta], real, total)


def bound(pats, counts, copies, passes: int) -> tuple[float, float, Run]:
    """(dev64, bound, the longdouble run) at ``passes`` updates: ``dev64`` is the largest absolute distance per allele of this
    file's float64 run from its longdouble run; another float64 evaluation of the same formulas (numpy's pairwise sums in the
    package) must lie within ``32 * max(dev64, 2^-52)`` of the longdouble run."""
    want = em(pats, counts, copies, passes=passes, dtype=LD)
    f64 = em(pats, counts, copies, passes=passes)
    dev64 = max(float(abs(LD(a) - b)) for a, b in zip(f64.theta, want.theta))
    return dev64, 32.0 * max(dev64, 2.0 ** -52), want
