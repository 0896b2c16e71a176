"""
EM ("report") strategy on the GPU -- drop-in for ``graphkir/typing_em.py``.

``hisat2TypingPerGene`` (191-215) becomes: candidate allele bit sets per read on the device
(``gk_em_sets`` = getCandidateAllelePerRead 68-87 + getMostFreqAllele 90-104), distinct sets with
multiplicities, SQUAREM EM in one workgroup (``gk_em_run`` = hisatEMnp 107-188).

Deviation (documented in DESIGN.md): ties in abundance are ordered by allele name here; the
reference orders them by the iteration order of a Python ``set`` (typing_em.py:213), which changes
from process to process.
"""
from __future__ import annotations

import ctypes as C
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from ._lib import DeviceBuffer, check, lib
from .engine import Tabulation


@dataclass
class Hisat2AlleleResult:
    """Abundance record of one allele (typing_em.py:21-28)."""

    allele: str
    count: int
    prob: float
    cn: int = 0


def candidateSets(tab: Tabulation, rows: DeviceBuffer, n_rows: int, vbeg: int, vend: int, mask: DeviceBuffer,
                  words: int) -> np.ndarray:
    """uint32 [n_rows][words] candidate-allele bit sets of the given rows."""
    out = tab.dev.alloc((max(n_rows, 1), words), np.uint32)
    check(lib().gk_em_sets(tab.dev.ctx, tab.handle, rows.ptr, n_rows, vbeg, vend, mask.ptr, words, out.ptr))
    sets = out.download()[:n_rows]
    out.free()
    return sets


def candidateSetsDistinct(tab: Tabulation, rows: DeviceBuffer, n_rows: int, vbeg: int, vend: int,
                          mask: DeviceBuffer, words: int) -> tuple[np.ndarray, np.ndarray]:
    """Distinct candidate-allele bit sets of the rows (ascending, like ``np.unique(axis=0)``) and their
    multiplicities; sets and grouping stay on the device, only the distinct ones come back."""
    buf = tab.dev.alloc((max(n_rows, 1), words), np.uint32)
    check(lib().gk_em_sets(tab.dev.ctx, tab.handle, rows.ptr, n_rows, vbeg, vend, mask.ptr, words, buf.ptr))
    cap = 1 << 14
    while True:
        sets = np.empty((cap, words), dtype=np.uint32)
        count = np.empty(cap, dtype=np.uint32)
        n = C.c_int32()
        rc = lib().gk_em_distinct(tab.dev.ctx, buf.ptr, n_rows, words, cap, sets.ctypes.data, count.ctypes.data, C.byref(n))
        if rc == -5 and cap < max(n_rows, 1):
            cap = min(cap * 16, max(n_rows, 1))
            continue
        check(rc)
        break
    buf.free()
    sets, count = sets[:n.value], count[:n.value].astype(np.int64)
    order = np.lexsort(sets.T[::-1]) if len(sets) else np.zeros(0, dtype=np.int64)   # rows ascending, word 0 first
    return np.ascontiguousarray(sets[order]), count[order]


_MIX = (np.arange(1, 65, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)


def distinctSets(sets: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Distinct rows (ascending, like ``np.unique(axis=0)``) and their multiplicities.

    Rows are grouped through a 64-bit mix of their words; the grouping is then verified against the
    rows themselves, and the exact (slow) path is taken in the unlikely case of a collision."""
    if len(sets) == 0:
        return sets.reshape(0, sets.shape[1]), np.zeros(0, dtype=np.int64)
    with np.errstate(over="ignore"):
        h = (sets.astype(np.uint64) * _MIX[:sets.shape[1]]).sum(axis=1, dtype=np.uint64)
        h ^= h >> np.uint64(29)
    _, first, inverse, counts = np.unique(h, return_index=True, return_inverse=True, return_counts=True)
    reps = sets[first]
    if not np.array_equal(reps[inverse], sets):
        return np.unique(sets, axis=0, return_counts=True)
    uniq, back = np.unique(reps, axis=0, return_inverse=True)
    weight = np.bincount(back.ravel(), weights=counts, minlength=len(uniq)).astype(np.int64)
    return uniq, weight


def hisatEMdevice(tab: Tabulation, sets, n_allele: int, iter_max: int = 300,
                  diff_threshold: float = 0.0001) -> tuple[np.ndarray, np.ndarray, int]:
    """Abundance per allele column, read count per allele, iterations used.

    ``sets``: the per-read bit sets, or the pair (distinct sets, multiplicities)."""
    uniq, weight = sets if isinstance(sets, tuple) else distinctSets(sets)
    words = uniq.shape[1]
    bits = np.unpackbits(uniq.view(np.uint8), axis=1, bitorder="little")[:, :n_allele]
    count = (bits.astype(np.int64) * weight[:, None]).sum(axis=0)      # reads naming each allele
    keep = uniq.any(axis=1)
    uniq, weight = np.ascontiguousarray(uniq[keep]), np.ascontiguousarray(weight[keep].astype(np.float64))
    prob = np.zeros(n_allele, dtype=np.float64)
    iters = C.c_int32(0)
    if len(uniq):
        check(lib().gk_em_run(tab.dev.ctx, uniq.ctypes.data, weight.ctypes.data, len(uniq), words, n_allele,
                              iter_max, diff_threshold, prob.ctypes.data, C.byref(iters)))
    return prob, count, int(iters.value)


def hisat2TypingPerGene(tab: Tabulation, rows: DeviceBuffer, n_rows: int, vbeg: int, vend: int, mask: DeviceBuffer,
                        words: int, alleles: list[str], info: dict | None = None) -> list[Hisat2AlleleResult]:
    """Per-gene EM report.  Raises like the reference when no read names any allele.  ``info`` (optional)
    receives ``iterations`` and ``distinct_sets``.  ``iterations`` is the number (from 0) of the SQUAREM pass whose
    difference met the 1e-4 stop, so 0 .. 299 for a run that stopped, and 300 (``iter_max``) for a run that did not:
    the reference returns no count, and its loop variable would read 299 both for a stop in the last pass and for none."""
    sets = candidateSetsDistinct(tab, rows, n_rows, vbeg, vend, mask, words)
    prob, count, iters = hisatEMdevice(tab, sets, len(alleles))
    if info is not None:
        info["iterations"], info["distinct_sets"] = iters, len(sets[0])
    named = np.nonzero(count)[0]
    return [Hisat2AlleleResult(allele=alleles[a], count=int(count[a]), prob=float(prob[a])) for a in named]


def callsByAbundance(alleles: list[str], prob: list[float], cn: int) -> tuple[list[str], list[int], list[int]]:
    """Abundances -> calls (kir_typing.py:181-192): the copy numbers go to the alleles in descending abundance, ties by
    allele name; an allele takes ``max(1, round(p * cn))`` copies until none are left.

    Returns the called alleles, the order the alleles were visited in (indices into ``alleles``; all of them) and the
    copies predicted for the visited ones (as many entries as were visited before the copies ran out)."""
    order = sorted(range(len(alleles)), key=lambda i: (-prob[i], alleles[i]))
    est_prob = 1 / cn
    called: list[str] = []
    pred: list[int] = []
    for i in order:
        k = max(1, round(float(prob[i]) / est_prob))
        called.extend([alleles[i]] * min(cn, k))
        pred.append(k)
        cn -= k
        if cn <= 0:
            break
    return called, order, pred


@dataclass
class EmBootstrap:
    """Read bootstrap of one gene's EM report: ``prob[b, a]`` is the abundance of ``alleles[a]`` (the alleles of the
    point report, in report order) in replicate ``b``, ``calls[b]`` the replicate's calls by the rule of the point call,
    ``call_support`` the share of replicates whose calls equal the point call as a multiset, ``rows`` the lines of
    ``{result}.confidence.tsv`` (one per allele: point values, replicate mean / sd / 2.5 % / 97.5 %, support)."""

    alleles: list[str]
    prob: np.ndarray
    iterations: np.ndarray
    calls: list[list[str]]
    call_support: float
    rows: list[dict] = field(default_factory=list)


CONFIDENCE_COLUMNS = ["gene", "allele", "cn", "count", "prob", "boot_mean", "boot_sd", "boot_lo", "boot_hi", "support",
                      "call_support"]


def bootstrapEM(tab, genes: list[tuple[np.ndarray, np.ndarray, int, int]], n_boot: int,
                seed: int, iter_max: int = 300, diff_threshold: float = 0.0001,
                want_counts: bool = False):
    """``n_boot`` bootstrap replicates of the EM of every gene in ONE ``gk_em_bootstrap`` call.

    ``genes``: (distinct sets uint32 [n_sets][words] ascending, multiplicities, alleles, stream number) per gene, the
    empty set included (``candidateSetsDistinct``).  Returns ``prob[n_boot, sum of alleles]`` (genes one after the
    other) and ``iterations[n_boot, genes]``; with ``want_counts`` also the replicate weights ``[n_boot, sum of sets]``."""
    from . import _lib
    jobs = (_lib.BootJob * max(len(genes), 1))()
    keep = []
    for q, (sets, count, n_allele, stream) in enumerate(genes):
        sets = np.ascontiguousarray(sets, dtype=np.uint32)
        assert sets.ndim == 2, "distinct sets: uint32 [n_sets][words]"
        count = np.asarray(count)
        if len(count) and (count.min() < 0 or int(count.sum()) >= 1 << 31):
            raise ValueError("bootstrapEM: multiplicities must be non-negative and sum to less than 2^31")
        count = np.ascontiguousarray(count, dtype=np.uint32)
        assert len(count) == len(sets)
        keep += [sets, count]
        jobs[q] = _lib.BootJob(sets=sets.ctypes.data, count=count.ctypes.data, n_sets=len(sets), words=max(sets.shape[1], 1),
                               n_allele=int(n_allele), stream=int(stream))
    total = sum(int(g[2]) for g in genes)
    n_sets = sum(len(g[1]) for g in genes)
    prob = np.zeros((n_boot, total), dtype=np.float64)
    iters = np.zeros((n_boot, len(genes)), dtype=np.int32)
    counts = np.zeros((n_boot, n_sets), dtype=np.uint32) if want_counts else None
    dev = getattr(tab, "dev", tab)      # a tabulation, or the device context itself
    check(lib().gk_em_bootstrap(dev.ctx, jobs, len(genes), n_boot,
                                int(seed) & 0xFFFFFFFFFFFFFFFF, iter_max, diff_threshold, prob.ctypes.data, iters.ctypes.data,
                                counts.ctypes.data if want_counts else None))
    del keep
    return (prob, iters, counts) if want_counts else (prob, iters)


def summariseBootstrap(gene: str, cn: int, report: list[Hisat2AlleleResult], called: list[str], alleles: list[str],
                       prob: np.ndarray, iterations: np.ndarray) -> EmBootstrap:
    """The derived numbers of one gene (host; B x A is small).  ``report``: the point report as ``_callsOfReport`` left
    it (sorted, copies filled in); ``called``: the point call; ``prob[B, len(alleles)]``: the replicates' abundances of
    ALL alleles of the gene.  A replicate's report is the point report's alleles with the replicate's abundances."""
    col = {a: i for i, a in enumerate(alleles)}
    names = [r.allele for r in report]
    x = np.ascontiguousarray(prob[:, [col[a] for a in names]], dtype=np.float64).reshape(len(prob), len(names))
    n_boot = len(x)
    calls = [callsByAbundance(names, x[b].tolist(), cn)[0] for b in range(n_boot)]
    point = Counter(called)
    tallies = [Counter(c) for c in calls]
    call_support = sum(t == point for t in tallies) / n_boot
    rows = []
    for i, rec in enumerate(report):
        need = max(1, point.get(rec.allele, 0))      # an allele that is not called: the replicates that call it at all
        lo, hi = np.percentile(x[:, i], [2.5, 97.5])
        rows.append({"gene": gene, "allele": rec.allele, "cn": int(rec.cn), "count": int(rec.count), "prob": float(rec.prob),
                     "boot_mean": float(x[:, i].mean()), "boot_sd": float(x[:, i].std(ddof=1)) if n_boot > 1 else 0.0,
                     "boot_lo": float(lo), "boot_hi": float(hi),
                     "support": sum(t.get(rec.allele, 0) >= need for t in tallies) / n_boot,
                     "call_support": call_support})
    return EmBootstrap(alleles=names, prob=x, iterations=np.asarray(iterations).copy(), calls=calls,
                       call_support=call_support, rows=rows)


def confidenceText(bootstrap: dict[str, EmBootstrap]) -> str:
    """``{result}.confidence.tsv``: tab separated, one row per allele of every gene's point report in report order,
    floats as ``repr(float)``."""
    lines = ["\t".join(CONFIDENCE_COLUMNS)]
    for boot in bootstrap.values():
        for row in boot.rows:
            lines.append("\t".join(str(row[k]) if isinstance(row[k], (str, int)) else repr(float(row[k]))
                                   for k in CONFIDENCE_COLUMNS))
    return "\n".join(lines) + "\n"
