"""
Read-bootstrap support of a likelihood call (``--call-bootstrap``).

The likelihood strategies rank allele sets by ``value = sum_r max_j L[r, ids[j]]`` (typing_mulit_allele.py:540-542) and
``.possible.tsv`` lists the sets within 10 % of the best -- but not whether that order would survive another draw of the
reads.  A replicate here RESCORES the candidate sets the point search ranked, with resampled read weights; no search,
fraction filter or zygosity test runs again:

1. candidates: the rows of the last step's ``TypingResult`` in rank order, repeats of an allele multiset dropped, the
   first ``top`` kept, the called row (``TypingResult.bestRank``) appended when it lies beyond;
2. ``V[t][r] = max_j L[r, ids[t][j]]`` on the table the search left in HBM (``gk_setmax``, ``DeviceModel.tableFor``);
3. ``W[b][r]`` = draws of replicate ``b`` on read ``r`` out of ``n_rows`` (``gk_boot_row_counts``: the generator of the EM
   bootstrap, stream = the gene's ordinal in the index; a replicate depends on (seed, b, stream, n_rows) alone);
4. ``S[b][t] = f * sum_r W[b][r] V[t][r]`` (``gk_weighted_sums``, one fixed summation order), ``f`` = the copy number for
   a result of ``createHomoResult`` -- so ``S`` is on the scale of ``value``;
5. the summary on the host (``summariseCall``): support = share of replicates a candidate wins, and the replicates' mean /
   2.5 % / 97.5 % of its distance to the called set.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .utils import logger

MAX_BOOT = 10000                 # replicates of one library call (include/graphkir_hip.h)
MAX_TOP = 256                    # candidate sets kept, and sets of one gk_weighted_sums call
V_BYTES = 512 << 20              # the per-read values of a slice of the sets
W_BYTES = 256 << 20              # the weights of a slice of the replicates

CALL_CONFIDENCE_COLUMNS = ["gene", "cn", "rank", "called", "value", "support", "delta_mean", "delta_q025", "delta_q975"]


@dataclass
class CallBootstrap:
    """Read bootstrap of one gene's call.  ``rows``: the candidates as rows of the typing result (rank order; the called
    row last when it lay beyond ``top``), ``called``: the position of the called set in ``rows``, ``value``: the point
    values, ``scores[b, t]``: candidate ``t`` rescored in replicate ``b``, ``support[t]``: share of replicates it wins,
    ``delta_*``: mean / 2.5 % / 97.5 % over the replicates of ``scores[:, t] - scores[:, called]`` (an interval that holds
    0: not separable from the call).  ``cn`` and ``alleles`` (the candidates' names) label the file's rows."""

    rows: np.ndarray
    called: int
    value: np.ndarray
    scores: np.ndarray
    support: np.ndarray
    delta_mean: np.ndarray
    delta_lo: np.ndarray
    delta_hi: np.ndarray
    cn: int = 0
    alleles: list[list[str]] = field(default_factory=list)

    @property
    def call_support(self) -> float:
        return float(self.support[self.called])


def summariseCall(scores: np.ndarray, called: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(support, delta_mean, delta_lo, delta_hi) of ``scores[B, T]`` (host; B x T is small): a replicate is won by its
    highest score, the lowest row among equal ones."""
    scores = np.asarray(scores, dtype=np.float64)
    n_boot, n_sets = scores.shape
    assert n_boot >= 1 and 0 <= called < n_sets
    winner = np.argmax(scores, axis=1)                     # the first of equal maxima
    support = np.bincount(winner, minlength=n_sets) / n_boot
    delta = scores - scores[:, [called]]
    lo, hi = np.percentile(delta, [2.5, 97.5], axis=0)
    return support, delta.mean(axis=0), lo, hi


def candidateRows(result, top: int) -> tuple[np.ndarray, int]:
    """(rows of ``result`` kept as candidates, position of the called row among them)."""
    ids = np.sort(np.asarray(result.allele_id, dtype=np.int64).reshape(len(result.value), -1), axis=1)
    _, first = np.unique(ids, axis=0, return_index=True)
    rows = np.sort(first)[:top]
    best = int(result.bestRank())
    first_of_best = int(np.flatnonzero((ids == ids[best]).all(axis=1))[0])    # the kept row with the called multiset
    at = np.flatnonzero(rows == first_of_best)
    if len(at):
        return rows, int(at[0])
    return np.append(rows, first_of_best), len(rows)


def homoFactor(result) -> int:
    """The factor between a result's ``value`` and the sum of its sets' per-read values: ``cn`` for a result made by
    ``createHomoResult`` (one-allele sets of the first step, values times cn), 1 otherwise."""
    parts = getattr(result.allele_prob, "parts", None)
    if parts and result.n > 1 and all(np.ndim(ids) == 2 and np.shape(ids)[1] == 1 for _, ids in parts):
        return int(result.n)
    return 1


def weightedScores(model, ids: np.ndarray, n_boot: int, seed: int, stream: int) -> np.ndarray:
    """``sum_r W[b][r] * max_j L[r, ids[t][j]]`` [n_boot, len(ids)] on ``model``'s table: per-read values of a slice of the
    sets (at most 256 sets and ``V_BYTES``), weights of a slice of the replicates (``W_BYTES``), one library call per pair
    of slices.  The slices are independent: the same bits however they are cut."""
    dev, n = model.dev, int(model.n_rows)
    table, ld, cols = model.tableFor(ids)
    n_sets, c = cols.shape
    set_slice = int(max(1, min(n_sets, MAX_TOP, V_BYTES // (8 * n))))
    boot_slice = int(max(1, min(n_boot, MAX_BOOT, W_BYTES // (4 * n))))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    scores = np.empty((n_boot, n_sets), dtype=np.float64)
    V = dev.alloc((set_slice, n), np.float64)
    W = dev.alloc((boot_slice, n), np.uint32)
    try:
        drawn = None                  # the replicates W holds
        for t0 in range(0, n_sets, set_slice):
            part = np.ascontiguousarray(cols[t0:t0 + set_slice])
            check(lib().gk_setmax(dev.ctx, table.ptr, n, ld, part.ctypes.data, len(part), c, V.ptr))
            for b0 in range(0, n_boot, boot_slice):
                nb = min(boot_slice, n_boot - b0)
                if drawn != (b0, nb):
                    check(lib().gk_boot_row_counts(dev.ctx, n, nb, b0, seed, int(stream), W.ptr, n))
                    drawn = (b0, nb)
                out = np.empty((nb, len(part)), dtype=np.float64)
                check(lib().gk_weighted_sums(dev.ctx, V.ptr, n, n, len(part), W.ptr, n, nb, out.ctypes.data))
                scores[b0:b0 + nb, t0:t0 + len(part)] = out
    finally:
        V.free()
        W.free()
    return scores


def bootstrapCall(result, cn_factor: int, n_boot: int, seed: int, stream: int, top: int = 32) -> CallBootstrap | None:
    """The read bootstrap of one gene's adopted result (the last step's ``TypingResult``); None -- with a warning --
    when the result's sets do not sit on one device table."""
    if not 1 <= int(top) <= MAX_TOP:
        raise ValueError(f"call bootstrap: top must lie in 1 .. {MAX_TOP}, got {top}")
    if int(n_boot) < 1:
        raise ValueError(f"call bootstrap: the number of replicates must be positive, got {n_boot}")
    model = modelOf(result)
    if model is None or not model.n_rows:
        logger.warning("[Allele] call bootstrap: the result's sets are not on one device table; skipped")
        return None
    rows, called = candidateRows(result, int(top))
    ids = np.asarray(result.allele_id, dtype=np.int64)[rows]
    scores = weightedScores(model, ids, int(n_boot), seed, stream)
    if cn_factor != 1:
        scores = scores * float(cn_factor)
    support, mean, lo, hi = summariseCall(scores, called)
    return CallBootstrap(rows=rows, called=called, value=np.asarray(result.value, dtype=np.float64)[rows], scores=scores,
                         support=support, delta_mean=mean, delta_lo=lo, delta_hi=hi, cn=int(result.n),
                         alleles=[list(result.allele_name[int(r)]) for r in rows])


def callConfidenceText(bootstrap: dict[str, CallBootstrap]) -> str:
    """``{result}.call_confidence.tsv``: tab separated, one row per candidate of every gene in candidate order, then the
    allele columns ``1 .. max cn`` as in ``.possible.tsv``; floats as ``repr(float)`` (``typing_em.confidenceText``)."""
    width = max((len(a) for boot in bootstrap.values() for a in boot.alleles), default=0)
    lines = ["\t".join(CALL_CONFIDENCE_COLUMNS + [str(i + 1) for i in range(width)])]
    for gene, boot in bootstrap.items():
        for t, row in enumerate(boot.rows):
            cells = [gene, str(int(boot.cn)), str(int(row)), str(int(t == boot.called))]
            cells += [repr(float(x[t])) for x in (boot.value, boot.support, boot.delta_mean, boot.delta_lo, boot.delta_hi)]
            names = list(boot.alleles[t])
            lines.append("\t".join(cells + names + [""] * (width - len(names))))
    return "\n".join(lines) + "\n"


# at the end, not at the top: call_report's table of reports names this module, and whichever of the two is imported first
# finds what it needs of the other already defined
from .call_report import modelOf  # noqa: E402
