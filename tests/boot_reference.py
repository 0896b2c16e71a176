"""CPU restatement of the EM read bootstrap (helper of the bootstrap tests, not a test).

Draw ``i`` of replicate ``b`` of stream ``g`` (64-bit wrapping arithmetic)::

    z  = seed + (i+1)*0x9E3779B97F4A7C15 + (b+1)*0xBF58476D1CE4E5B9 + (g+1)*0x94D049BB133111EB
    z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
    j  = ((z >> 32) * n) >> 32

and draw ``j`` belongs to the set ``u`` with ``cum[u] <= j < cum[u + 1]`` (``cum``: prefix sums of the multiplicities).
"""
from __future__ import annotations

import numpy as np

_C1, _C2, _C3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def draws(seed: int, g: int, b: int, n: int) -> np.ndarray:
    """The ``n`` draws (read numbers below ``n``) of replicate ``b`` of stream ``g``."""
    assert 0 <= n < 1 << 31
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + i * _C1 + np.uint64(b + 1) * _C2 + np.uint64(g + 1) * _C3
        z ^= z >> np.uint64(30)
        z *= _C2
        z ^= z >> np.uint64(27)
        z *= _C3
        z ^= z >> np.uint64(31)
        return ((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def replicateCounts(seed: int, g: int, b: int, count) -> np.ndarray:
    """Replicate weights of the sets with multiplicities ``count`` (int64 [n_sets]; they sum to ``sum(count)``)."""
    count = np.asarray(count, dtype=np.int64)
    cum = np.cumsum(count)
    n = int(cum[-1]) if len(cum) else 0
    if n == 0:
        return np.zeros(len(count), dtype=np.int64)
    at = np.searchsorted(cum, draws(seed, g, b, n).astype(np.int64), side="right")
    return np.bincount(at, minlength=len(count)).astype(np.int64)


def replicateReads(sets: np.ndarray, weights, alleles: list[str]) -> list[list[str]]:
    """The replicate as per-read allele-name lists for ``oracle.em.squaremEM``: set ``u`` (uint32 bit words, bit ``a`` of
    the row = ``alleles[a]``) repeated ``weights[u]`` times; the empty set gives reads that name nobody."""
    bits = np.unpackbits(np.ascontiguousarray(sets, dtype=np.uint32).view(np.uint8), axis=1, bitorder="little")
    reads: list[list[str]] = []
    for row, w in zip(bits[:, :len(alleles)], weights):
        names = [alleles[a] for a in np.nonzero(row)[0]]
        reads.extend([names] * int(w))
    return reads
