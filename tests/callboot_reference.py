"""CPU restatement of the call bootstrap of the likelihood strategies (helper of its tests, not a test): the replicate
weights per read from the draws of tests/boot_reference.py, and the rescored sets as a plain matrix product."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import boot_reference  # noqa: E402


def rowCounts(seed: int, g: int, b: int, n: int) -> np.ndarray:
    """``w_b[r]``: how many of the ``n`` draws of replicate ``b`` of stream ``g`` fall on read ``r`` (int64 [n])."""
    return np.bincount(boot_reference.draws(seed, g, b, n).astype(np.int64), minlength=n)


def weights(seed: int, g: int, boots, n: int) -> np.ndarray:
    """``rowCounts`` of the listed replicates [len(boots), n]."""
    return np.array([rowCounts(seed, g, b, n) for b in boots], dtype=np.int64).reshape(len(boots), n)


def scores(W: np.ndarray, V: np.ndarray) -> np.ndarray:
    """``S[b][t] = sum_r W[b][r] * V[t][r]`` (W [B, n], V [T, n])."""
    return W.astype(np.float64) @ np.asarray(V, dtype=np.float64).T
